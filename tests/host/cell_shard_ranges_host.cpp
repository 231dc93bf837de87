// Host build of kzg_rs_amd/csrc/cell_shard_ranges.hpp for tests/test_cell_shard_ranges_cpu.py: the ranges a multi-device handle
// cuts a cell call into, as the library computes them.
#include "cell_shard_ranges.hpp"
using namespace kzg;
extern "C" {
// out[2 k], out[2 k + 1] = shard k's range [lo, hi); weights == nullptr: units of equal weight (ceil(n / D) per shard)
void h_shard_ranges(const size_t* weights, size_t n, size_t D, size_t* out) {
    std::vector<CellShardRange> r;
    if (weights) cell_shard_ranges_weighted(r, weights, n, D);
    else cell_shard_ranges_even(r, n, D);
    for (size_t k = 0; k < r.size(); k++) out[2 * k] = r[k].lo, out[2 * k + 1] = r[k].hi;
}
}
