// Stand-alone driver of kzg_rs_amd/csrc/fr_ntt_plan.hpp (tests/test_fr_ntt_plan_cpu.py builds it with g++ and
// -fsanitize=address,undefined): it walks the passes the way the kernels of fr_ntt_kernels.hpp do, into arrays the sanitizers watch,
// and prints what the header computes; the test compares with its own arithmetic.
//   geometry                     -> "tile threads max chunk_elems table bad_flag"
//   shapes                       -> per k in 0..20: "k k1 k2 passes"
//   maps k polys brp_in brp_out  -> per pass: "kind tiles log2_len loads_once lds_in_once stores_once lds_out_once max_e"
//   chunks n n_polys             -> "chunk n_chunks" then per chunk (one behind the last too) "lo m io_bytes scratch_scalars tiles"
//   bfly                         -> per stage (half = 1 .. tile / 2): "half once max_e": every element of the tile in exactly one butterfly
//   ntt k polys inverse order in -> the transform of the polys x 2^k values of file `in` (64 hex digits a line, big-endian), composed
//                                   as the kernels compose it: "top limb" (the largest top limb and the largest lower limb any stage
//                                   output had), then the results, one a line
//   nttbin k polys inverse order in out -> the same with the values as 32 big-endian bytes each in file `in`, the results likewise in
//                                   file `out`; "top limb" alone is printed (the sizes whose values as text would be 100 MB)
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fr_ntt_plan.hpp"
using namespace kzg;

typedef std::array<uint32_t, 8> Words;

static uint32_t g_top = 0, g_limb = 0;
static void watch(const Fr29& a) {
    if (a.l[8] > g_top) g_top = a.l[8];
    for (int i = 0; i < 8; i++)
        if (a.l[i] > g_limb) g_limb = a.l[i];
}

// one launch of k_fr_ntt_pass<kind>: src and dst hold exactly `total` elements
static void run_pass(int kind, const std::vector<Words>& src, std::vector<Words>& dst, const std::vector<Fr29>& W, int k, size_t total, bool perm_in, bool perm_out,
                     bool inverse, const Fr29& scale) {
    const FrNttShape sh = frntt_shape(k);
    for (size_t tile = 0; tile < frntt_tiles(total); tile++) {
        std::vector<Fr29> s(FRNTT_TILE);
        for (uint32_t x = 0; x < FRNTT_TILE; x++) {
            const FrNttSlot a = frntt_load(kind, sh, total, tile, x, perm_in);
            Fr29 v = frntt_small(0u);
            if (a.live) {
                uint32_t w[8];
                for (int i = 0; i < 8; i++) w[i] = src[a.at][i];
                v = fr29_from_words(w);
            }
            s[a.lds] = v;
        }
        const int len = 1 << frntt_pass_log2(sh, kind);
        for (int half = 1; half < len; half <<= 1)
            for (int j = 0; j < (int)FRNTT_TILE / 2; j++) {
                const FrNttBfly b = frntt_bfly(j, half, inverse);
                cell_ntt_apply(s[b.i0], s[b.i1], W[b.e]);
                watch(s[b.i0]);
                watch(s[b.i1]);
            }
        // (all loads of a tile come before its first store: src may be dst)
        for (uint32_t x = 0; x < FRNTT_TILE; x++) {
            const FrNttSlot a = frntt_store(kind, sh, total, tile, x, perm_out, inverse);
            if (!a.live) continue;
            uint32_t w[8];
            if (kind == FRNTT_COLUMNS)
                fr29_to_words(w, frntt_twiddle(s[a.lds], W[a.e >> FRNTT_TILE_LOG2], W[FRNTT_TABLE + (a.e & (FRNTT_TABLE - 1))]));
            else
                frntt_canonical(w, s[a.lds], scale);
            for (int i = 0; i < 8; i++) dst[a.at][i] = w[i];
        }
    }
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "geometry")) {
        printf("%zu %zu %zu %zu %d %u\n", FRNTT_TILE, FRNTT_THREADS, FRNTT_MAX, FRNTT_CHUNK_ELEMS, FRNTT_TABLE, FRNTT_BAD_ELEMENT);
        return 0;
    }
    if (!strcmp(argv[1], "shapes")) {
        for (int k = 0; k <= FRNTT_MAX_LOG2; k++) {
            const FrNttShape sh = frntt_shape(k);
            if (frntt_log2((size_t)1 << k) != k || frntt_log2(((size_t)1 << k) + 1) != (k ? -1 : 1) || frntt_log2(0) != -1) return 3;
            printf("%d %d %d %d\n", sh.k, sh.k1, sh.k2, sh.passes);
        }
        return 0;
    }
    if (!strcmp(argv[1], "maps") && argc == 6) {
        const int k = atoi(argv[2]);
        const size_t polys = strtoull(argv[3], nullptr, 10), total = polys << k;
        const bool brp_in = atoi(argv[4]) != 0, brp_out = atoi(argv[5]) != 0;
        const FrNttShape sh = frntt_shape(k);
        for (int pass = 0; pass < sh.passes; pass++) {
            const int kind = sh.passes == 1 ? FRNTT_SINGLE : (pass ? FRNTT_ROWS : FRNTT_COLUMNS);
            std::vector<uint8_t> ld(total, 0), st(total, 0);  // (exactly total: an index at total or above is a sanitizer report)
            bool lds_in = true, lds_out = true;
            uint32_t max_e = 0;
            for (size_t W = 0; W < frntt_tiles(total); W++) {
                std::vector<uint8_t> li(FRNTT_TILE, 0), lo(FRNTT_TILE, 0);
                for (uint32_t x = 0; x < FRNTT_TILE; x++) {
                    const FrNttSlot a = frntt_load(kind, sh, total, W, x, kind != FRNTT_ROWS && brp_in);
                    li[a.lds]++;
                    if (a.live) ld[a.at]++;
                    const FrNttSlot b = frntt_store(kind, sh, total, W, x, kind != FRNTT_COLUMNS && brp_out, true);
                    lo[b.lds]++;
                    if (b.live) st[b.at]++;
                    if (b.e > max_e) max_e = b.e;
                }
                for (size_t i = 0; i < FRNTT_TILE; i++) lds_in = lds_in && li[i] == 1, lds_out = lds_out && lo[i] == 1;
            }
            bool loads = true, stores = true;
            for (size_t i = 0; i < total; i++) loads = loads && ld[i] == 1, stores = stores && st[i] == 1;
            printf("%d %zu %d %d %d %d %d %u\n", kind, frntt_tiles(total), frntt_pass_log2(sh, kind), (int)loads, (int)lds_in, (int)stores, (int)lds_out, max_e);
        }
        return 0;
    }
    if (!strcmp(argv[1], "chunks") && argc == 4) {
        const size_t n = strtoull(argv[2], nullptr, 10), n_polys = strtoull(argv[3], nullptr, 10);
        const size_t chunk = n_polys < frntt_chunk_polys(n) ? n_polys : frntt_chunk_polys(n);
        printf("%zu %zu\n", chunk, frntt_chunks(n_polys, chunk));
        for (size_t c = 0; c <= frntt_chunks(n_polys, chunk); c++) {
            const size_t lo = frntt_chunk_lo(c, chunk), m = frntt_chunk_size(n_polys, c, chunk);
            printf("%zu %zu %zu %zu %zu\n", lo, m, frntt_io_bytes(n, m), frntt_scratch_scalars(n, m), frntt_tiles(n * m));
        }
        return 0;
    }
    if (!strcmp(argv[1], "bfly")) {
        for (int half = 1; half < (int)FRNTT_TILE; half <<= 1) {
            std::vector<uint8_t> seen(FRNTT_TILE, 0);
            uint32_t max_e = 0;
            bool once = true;
            for (int j = 0; j < (int)FRNTT_TILE / 2; j++) {
                const FrNttBfly f = frntt_bfly(j, half, false), b = frntt_bfly(j, half, true);
                seen[f.i0]++, seen[f.i1]++;
                once = once && f.i1 == f.i0 + half && b.i0 == f.i0 && ((f.e + b.e) & (FRNTT_TABLE - 1)) == 0;
                if (f.e > max_e) max_e = f.e;
                if (b.e > max_e) max_e = b.e;
            }
            for (size_t i = 0; i < FRNTT_TILE; i++) once = once && seen[i] == 1;
            printf("%d %d %u\n", half, (int)once, max_e);
        }
        return 0;
    }
    const bool bin = !strcmp(argv[1], "nttbin") && argc == 8;
    if ((!strcmp(argv[1], "ntt") && argc == 7) || bin) {
        const int k = atoi(argv[2]);
        if (k < 0 || k > FRNTT_MAX_LOG2) return 2;
        const size_t polys = strtoull(argv[3], nullptr, 10), total = polys << k;
        const bool inverse = atoi(argv[4]) != 0, brp = atoi(argv[5]) != 0;
        std::vector<Words> io(total), tmp(frntt_scratch_scalars((size_t)1 << k, polys));
        FILE* f = fopen(argv[6], bin ? "rb" : "r");
        if (!f) return 4;
        char line[128];
        for (size_t i = 0; i < total; i++) {
            if (bin) {
                uint8_t be[32];
                if (fread(be, 1, 32, f) != 32) return 5;
                for (int wd = 0; wd < 8; wd++)
                    io[i][7 - wd] = (uint32_t)be[4 * wd] << 24 | (uint32_t)be[4 * wd + 1] << 16 | (uint32_t)be[4 * wd + 2] << 8 | (uint32_t)be[4 * wd + 3];
                continue;
            }
            if (!fgets(line, sizeof line, f) || strlen(line) < 64) return 5;
            for (int wd = 0; wd < 8; wd++) {
                char h[9];
                memcpy(h, line + 8 * wd, 8);
                h[8] = 0;
                io[i][7 - wd] = (uint32_t)strtoul(h, nullptr, 16);
            }
        }
        fclose(f);
        std::vector<Fr29> W(2 * FRNTT_TABLE);
        const Fr29 g = frntt_root_entry();
        for (int t = 0; t < 2 * FRNTT_TABLE; t++) W[t] = frntt_table_entry(g, (uint32_t)t & (FRNTT_TABLE - 1), t < FRNTT_TABLE);
        const Fr29 scale = frntt_scale_entry(k, inverse);
        const bool perm_in = brp && inverse, perm_out = brp && !inverse;
        if (frntt_shape(k).passes == 1) {
            run_pass(FRNTT_SINGLE, io, io, W, k, total, perm_in, perm_out, inverse, scale);
        } else {
            run_pass(FRNTT_COLUMNS, io, tmp, W, k, total, perm_in, false, inverse, scale);
            run_pass(FRNTT_ROWS, tmp, io, W, k, total, false, perm_out, inverse, scale);
        }
        printf("%u %u\n", g_top, g_limb);
        if (bin) {
            FILE* o = fopen(argv[7], "wb");
            if (!o) return 4;
            for (size_t i = 0; i < total; i++) {
                uint8_t be[32];
                for (int wd = 0; wd < 8; wd++)
                    for (int b = 0; b < 4; b++) be[4 * wd + b] = (uint8_t)(io[i][7 - wd] >> (24 - 8 * b));
                if (fwrite(be, 1, 32, o) != 32) return 6;
            }
            return fclose(o) ? 6 : 0;
        }
        for (size_t i = 0; i < total; i++) {
            for (int wd = 7; wd >= 0; wd--) printf("%08x", io[i][wd]);
            printf("\n");
        }
        return 0;
    }
    return 2;
}
