"""Helpers shared by the cell-prover tests: the test blobs, the FK20 index algebra over a scalar stand-in, and the host build of
kzg_rs_amd/csrc/cell_ntt.hpp."""
import ctypes as C
import os
import random
import subprocess

import cell_model as M
import golden_data as G

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
R = M.R
RP = 1 << 261
MASK = (1 << 29) - 1


def mainnet_blobs(k=2):
    rich = [t for t in G.valid_blob_tuples() if len(set(t[0][i:i + 32] for i in range(0, 4096 * 32, 32))) > 64]
    return [rich[i][0] for i in range(k)]


def random_blob(seed):
    rng = random.Random(seed)
    return M.to_bytes(rng.randrange(R) for _ in range(4096))


def zero_blob():
    return bytes(32 * 4096)


def constant_blob(v=0x1234567):
    return M.to_bytes([v] * 4096)


def top_degree_blob():
    """the blob whose polynomial is X^4095"""
    return M.evaluations([0] * 4095 + [1])


def max_blob():
    return M.to_bytes([R - 1] * 4096)


def numpy_blobs(seed, k):
    """k seeded canonical blobs as one uint8 array [k][131072]: random bytes, the top byte of every element masked to six bits,
    so every element is below 2^254 < r (one generator call where random_blob makes 4096 randrange calls per blob)."""
    import numpy as np
    a = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, size=(k, 4096, 32), dtype=np.uint8)
    a[:, :, 0] &= 0x3F
    return a.reshape(k, 32 * 4096)


# ---------------------------------------------------------------- the shapes of g1_msm_core, and the cell batches that sit on their seams
def g1_msm_constants():
    """(slice terms, first layer count of the large tail), read from csrc/capi_pieces.hpp: a changed constant moves the result of
    msm_shape and with it fails the size table's test, where a copy kept here would leave the sizes beside their seams."""
    import re
    src = open(os.path.join(ROOT, "kzg_rs_amd", "csrc", "capi_pieces.hpp")).read()
    slice_terms = re.search(r"constexpr\s+size_t\s+G1_MSM_SLICE_TERMS\s*=\s*(\d+)\s*;", src)
    tail = re.search(r"large_tail\s*=\s*gz\s*>=\s*(\d+)\s*&&", src)
    assert slice_terms and tail, "capi_pieces.hpp no longer states the slice constant or the large tail's threshold in this form"
    return int(slice_terms.group(1)), int(tail.group(1))


def msm_shape(n, slice_terms=None, tail_layers=None):
    """g1_msm_core's launch shape for a sum of n terms -> (S, gz, large_tail_by_layers): the terms go to two outputs of
    h = (n + 1) / 2 and n - h terms, each cut into S = ceil(h / slice_terms) slices, S rounded up to a multiple of 4 when above 1;
    the window grid has gz = 2 S layers, and from tail_layers layers on the sum ends in the bucket-by-bucket large tail (while
    the save area holds the whole grid: a layer is 8 x (256 x 48 + 1) words = 393 248 bytes, msm_save_reserve grows the area to
    min(layers x that, 512 MiB), so every grid of up to 1 365 layers - about 4 M terms - is admitted)."""
    if slice_terms is None or tail_layers is None:
        slice_terms, tail_layers = g1_msm_constants()
    h = (n + 1) // 2
    S = -(-h // slice_terms)
    S = 1 if S <= 1 else (S + 3) & ~3
    return S, 2 * S, 2 * S >= tail_layers


CELL_SIZE_BLOBS = 193   # blobs of the size tests' fixture; a triple (blob b, cell c) has the id 128 b + c


def _ids_blobs(nb, drop=False):
    import numpy as np
    ids = np.arange(128 * nb, dtype=np.int64)
    if drop:  # one cell index left out per blob, another one for each
        ids = ids[(ids & 127) != (7 * (ids >> 7) + 3) % 128]
    return ids


def _ids_repeat(nb):
    import numpy as np
    ids = _ids_blobs(nb)
    return np.concatenate([ids, ids[1000:1001]])


def _ids_column(col):
    import numpy as np
    return 128 * np.arange(CELL_SIZE_BLOBS, dtype=np.int64) + col


def _ids_shuffled_repeated():
    import numpy as np
    ids = np.random.Generator(np.random.PCG64(8192)).permutation(_ids_blobs(64))
    return np.resize(ids, 128 * CELL_SIZE_BLOBS)


# (id, triple ids, n, N, class of LL = the sum over n proofs, class of RL = the sum over N = n + m + 64 points); classes: "one" =
# one slice per output, no fold; "sliced" = S > 1, the slices' window sums folded by trees; "tail" = sliced, the large tail
CELL_SIZES = [
    ("48x127", lambda: _ids_blobs(48, drop=True), 6096, 6208, "one", "sliced"),
    ("48x128", lambda: _ids_blobs(48), 6144, 6256, "one", "sliced"),
    ("48x128+1", lambda: _ids_repeat(48), 6145, 6257, "sliced", "sliced"),
    ("64x128", lambda: _ids_blobs(64), 8192, 8320, "sliced", "sliced"),
    ("192x128", lambda: _ids_blobs(192), 24576, 24832, "sliced", "tail"),
    ("193x128", lambda: _ids_blobs(193), 24704, 24961, "tail", "tail"),
    ("column77", lambda: _ids_column(77), 193, 450, "one", "one"),
    ("64x128-shuffled-x3", _ids_shuffled_repeated, 24704, 24832, "tail", "tail"),
]


def cell_size_ids(name):
    return next(row[1] for row in CELL_SIZES if row[0] == name)()


def msm_class(n):
    S, gz, tail = msm_shape(n)
    return "one" if S == 1 else "tail" if tail else "sliced"


def cell_batch(cms, cells, proofs, ids):
    """The four arguments of kzg_verify_cell_kzg_proof_batch for the triples `ids`, gathered from the fixture's arrays
    (cms [blobs][48], cells and proofs [128 blobs][2048 | 48]) as contiguous arrays: [commitments, cell indices, cells, proofs]"""
    import numpy as np
    ids = np.asarray(ids, dtype=np.int64)
    return [cms[ids >> 7], (ids & 127).astype(np.uint64), cells[ids], proofs[ids]]


def verify_cells_raw(api, handle, args):
    """kzg_verify_cell_kzg_proof_batch itself on the arrays of cell_batch -> (return code, verdict)"""
    import numpy as np
    cm, idx, ce, pr = (np.ascontiguousarray(a) for a in args)
    assert cm.dtype == ce.dtype == pr.dtype == np.uint8 and idx.dtype == np.uint64
    n = len(idx)
    assert cm.shape == (n, 48) and ce.shape == (n, 2048) and pr.shape == (n, 48)
    ok = C.c_bool(False)
    rc = api.lib().kzg_verify_cell_kzg_proof_batch(C.byref(ok), cm.ctypes.data_as(C.c_char_p), idx.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                   ce.ctypes.data_as(C.c_char_p), pr.ctypes.data_as(C.c_char_p), n, handle)
    return rc, bool(ok.value)


def fk20_scalar_proofs(a, tau):
    """The 128 cell proofs of the polynomial with coefficients a, with [tau^m]G1 replaced by the scalar tau^m: the index algebra
    of include/kzg_rs_amd.h (set-up sums X, the 64 vectors t and their 128-point DFTs, H, and the inverse DFT - truncate - DFT
    written as the circulant it is: P[k] = H[k] / 2 + sum over odd d of H[k - d] / (64 (1 - w^d)))."""
    w = pow(M.W8192, 64, R)
    mono = [pow(tau, m, R) for m in range(4096)]
    X = [[sum(pow(w, j * k, R) * mono[4031 - i - 64 * j] for j in range(63)) % R for k in range(128)] for i in range(64)]
    H = [0] * 128
    for i in range(64):
        t = [0] * 128
        t[0] = a[4095 - i]
        for m in range(66, 128):
            t[m] = a[64 * (m - 64) - 1 - i]
        th = M._ntt(t, w)
        for k in range(128):
            H[k] = (H[k] + th[k] * X[i][k]) % R
    c = circulant()
    P = [sum(c[d] * H[(k - d) % 128] for d in c) % R for k in range(128)]
    return [P[M.brp(cc, 7)] for cc in range(128)]


def circulant():
    """d -> c[d]: the non-zero entries of the first column of F trunc F^-1 (128-point DFT, upper half dropped)"""
    w = pow(M.W8192, 64, R)
    c = {0: pow(2, R - 2, R)}
    for d in range(1, 128, 2):
        c[d] = pow(64 * (1 - pow(w, d, R)) % R, R - 2, R)
    return c


def words(xs):
    out = []
    for x in xs:
        out += [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    return (C.c_uint32 * len(out))(*out)


def unwords(buf, n):
    return [sum(int(buf[8 * i + k]) << (32 * k) for k in range(8)) for i in range(n)]


def twiddle_table():
    out, x = [], 1
    for _ in range(8192):
        v = x * RP % R
        out += [(v >> (29 * i)) & MASK for i in range(9)]
        x = x * M.W8192 % R
    return (C.c_uint32 * len(out))(*out)


def ntt_host_lib():
    out = os.path.join(HERE, "host", "_cell_ntt_host.so")
    src = os.path.join(HERE, "host", "cell_ntt_host.cpp")
    inc = os.path.join(ROOT, "kzg_rs_amd", "csrc")
    deps = [src, os.path.join(inc, "cell_ntt.hpp"), os.path.join(inc, "fr29.hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", inc, "-o", out, src])
    return C.CDLL(out)
