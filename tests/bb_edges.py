"""Edge values for the BabyBear commit path (sp1_amd/csrc/bb31.hpp, babybear.hip), chosen in the STORED (Montgomery) domain,
which is what a kernel sees: 0, the Montgomery one and its negative, p - 1 = 0x78000000, the values around p / 2, and words
whose 16-bit halves are 0 or 0xffff under the largest high half. Shared by tests/test_bb31_arith.py (the header, operation by
operation) and tests/test_gpu_bb_edges.py (the kernels through the C ABI)."""
import functools

import numpy as np

import bb_py

P = 0x78000001
R = 1 << 32
R_INV = pow(R, -1, P)
R1 = R % P
V16 = 0x77FFFFFF            # low half 0xffff under the largest high half
assert P == 2 ** 31 - 2 ** 27 + 1 == bb_py.P and R1 == 0x0FFFFFFE

EDGE_WORDS = [0, 1, 2, R1, P - R1, P - 2, P - 1, (P - 1) // 2, (P + 1) // 2, 0xFFFF, 0x10000, 0x00FFFFFF, 0x01000000, V16, 0x77FF0000]
assert all(w < P for w in EDGE_WORDS) and P - 1 == 0x78000000


def canon(words):
    """from_monty of an array of stored words: numpy uint64 (a word times 2^-32 mod p is < 2^62)."""
    return np.asarray(words).astype(np.uint64) * np.uint64(R_INV) % np.uint64(P)


def stored(values):
    """to_monty of an array of canonical values."""
    return ((np.asarray(values).astype(np.uint64) << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def edge_states():
    """[n][16] stored words: all 0, all p - 1, all 0x77ffffff, s[0] = 0 over p - 1 elsewhere and the reverse, one non-zero
    lane at each of the 16 positions, alternating 0 / p - 1 (both phases), 4096 states drawn from the pool, 4096 random."""
    rng = np.random.default_rng(3127)
    fixed = [[0] * 16, [P - 1] * 16, [V16] * 16, [0] + [P - 1] * 15, [P - 1] + [0] * 15, [0, P - 1] * 8, [P - 1, 0] * 8]
    for lane in range(16):
        for w in (P - 1, R1, V16):
            fixed.append([w if i == lane else 0 for i in range(16)])
    pool = np.array(EDGE_WORDS, dtype=np.uint32)
    out = np.concatenate([np.array(fixed, dtype=np.uint32), pool[rng.integers(0, len(pool), (4096, 16))],
                          rng.integers(0, P, (4096, 16)).astype(np.uint32)])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def permuted_edge_states():
    """bb_py's permutation of edge_states(), as stored words (computed once and shared)."""
    out = stored(bb_py.permute_many(canon(edge_states())))
    out.setflags(write=False)
    return out


# lg_n of the RS-encode edge test, each under log_blowup 0, 1, 2: every lg_n in 0..13, plus 15 and 16, and 17 for log N = 19
RS_EDGE_LG_N = list(range(0, 14)) + [15, 16, 17]
RS_EDGE_LOG_BLOWUPS = (0, 1, 2)


def pool_tensor(shape, seed):
    rng = np.random.default_rng(seed)
    pool = np.array(EDGE_WORDS, dtype=np.uint32)
    return pool[rng.integers(0, len(pool), shape)]


def ntt_columns(lg_n):
    """[n][2 lg_n + 7] stored words: all 0, all p - 1, 0 / p - 1 alternating at stride 2^k for every k < lg_n in both phases
    (x = 0 and y = p - 1 meet in one butterfly at the stage of that stride, and the reverse), single non-zero words at rows
    0, n - 1, n / 2 and n / 3."""
    n = 1 << lg_n
    cols = [np.zeros(n, np.uint32), np.full(n, P - 1, np.uint32)]
    i = np.arange(n)
    for k in range(lg_n):
        cols.append(np.where((i >> k) & 1, P - 1, 0).astype(np.uint32))
        cols.append(np.where((i >> k) & 1, 0, P - 1).astype(np.uint32))
    for idx, w in ((0, P - 1), (n - 1, P - 1), (n // 2, V16), (n // 3, R1), (n - 1, 1)):
        d = np.zeros(n, np.uint32)
        d[idx] = w
        cols.append(d)
    return np.stack(cols, axis=1)


def split_width(width):
    """Tensor widths summing to `width` whose boundaries fall inside a rate block of 8 (at 3, and at 11 and 113 when wide enough)."""
    if width < 4:
        return [width]
    if width < 12:
        return [3, width - 3]
    if width < 120:
        return [3, 8, width - 11]
    return [3, 8, 102, width - 113]
