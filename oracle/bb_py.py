"""Pure-Python BabyBear model of the commit path (TEST INFRASTRUCTURE ONLY — never imported by the product).

A second reference beside oracle/bb_commit.hpp, written from the definitions and independent of it in formulation: canonical
integers mod p = 2^31 - 2^27 + 1, no Montgomery words, no 64-bit tricks, the linear layers as explicit matrices, the DFT as
the naive sum. What it restates (the published Poseidon2 / Plonky3 BabyBear parameters the C++ oracle's header cites):

* field: p = 2^31 - 2^27 + 1, two-adicity 27, multiplicative generator 31
* Poseidon2 width 16, x^7, 8 external + 13 internal rounds; external layer circ(2 M4, M4, M4, M4) with
  M4 = [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]; internal layer (1 + diag(d)) 2^-32 with
  d = [-2, 1, 2, 4, ..., 2^13, 2^15] and 1 the all-ones matrix (UNPINNED by the reference tree, as in bb_commit.hpp: the
  published convention); round constants from bb_poseidon2_rc.inc in the order ext[0..3] | internal[0..12] | ext[4..7]
* PaddingFreeSponge<16, 8, 8> (a non-empty tail overwrites the first lanes of the previous state and is permuted; nothing is
  padded), TruncatedPermutation compression, commitment = compress(root, hash([log_height, total_width]))
* RS encode: out[bitrev(k)] = sum_i in[i] w_N^(k i), w_N = two_adic_generator(log N)
"""
import os
import re

P = 2 ** 31 - 2 ** 27 + 1
TWO_ADICITY = 27
GENERATOR = 31
R_INV = pow(1 << 32, -1, P)           # the 2^-32 factor of the internal layer

_HERE = os.path.dirname(os.path.abspath(__file__))


def _load_rc():
    txt = open(os.path.join(_HERE, "bb_poseidon2_rc.inc")).read()
    vals = [int(h, 16) for h in re.findall(r"0x([0-9a-f]{8})u", txt)]
    assert len(vals) == 30 * 16 and all(v < P for v in vals)
    return [vals[r * 16:(r + 1) * 16] for r in range(30)]


RC = _load_rc()
RC_EXTERNAL = RC[0:4] + RC[17:21]                 # four rounds before and four after the internal rounds
RC_INTERNAL = [RC[4 + r][0] for r in range(13)]

M4 = [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]
EXTERNAL_MATRIX = [[(2 if i // 4 == j // 4 else 1) * M4[i % 4][j % 4] for j in range(16)] for i in range(16)]
INTERNAL_DIAG = [-2] + [1 << k for k in range(14)] + [1 << 15]
INTERNAL_MATRIX = [[(1 + (INTERNAL_DIAG[i] if i == j else 0)) * R_INV % P for j in range(16)] for i in range(16)]


def two_adic_generator(bits):
    assert 0 <= bits <= TWO_ADICITY
    return pow(GENERATOR, (P - 1) >> bits, P)


def _matvec(m, s):
    return [sum(a * b for a, b in zip(row, s)) % P for row in m]


def external_linear(s):
    return _matvec(EXTERNAL_MATRIX, s)


def internal_linear(s):
    return _matvec(INTERNAL_MATRIX, s)


def sbox(x):
    return pow(x, 7, P)


def permute(state):
    s = external_linear([int(x) % P for x in state])
    for r in range(4):
        s = external_linear([sbox(s[i] + RC_EXTERNAL[r][i]) for i in range(16)])
    for r in range(13):
        s[0] = sbox(s[0] + RC_INTERNAL[r])
        s = internal_linear(s)
    for r in range(4, 8):
        s = external_linear([sbox(s[i] + RC_EXTERNAL[r][i]) for i in range(16)])
    return s


def matvec_many(m, s):
    """Row-wise m s for an [n][16] uint64 array of canonical values: every product (< 2^62) is reduced before the sum."""
    import numpy as np
    return (s[:, None, :] * np.array(m, dtype=np.uint64)[None, :, :] % np.uint64(P)).sum(axis=2) % np.uint64(P)


def sbox_many(x):
    import numpy as np
    p = np.uint64(P)
    x2 = x * x % p
    x4 = x2 * x2 % p
    return x4 * x2 % p * x % p


def permute_many(states):
    """`permute` on every row of an [n][16] array at once (numpy uint64, the same matrices and constants): for the tests that
    hold thousands of states. tests/test_bb31_arith.py holds it equal to `permute`."""
    import numpy as np
    p = np.uint64(P)
    s = matvec_many(EXTERNAL_MATRIX, np.asarray(states, dtype=np.uint64) % p)
    for r in range(4):
        s = matvec_many(EXTERNAL_MATRIX, sbox_many((s + np.array(RC_EXTERNAL[r], dtype=np.uint64)) % p))
    for r in range(13):
        s[:, 0] = sbox_many((s[:, 0] + np.uint64(RC_INTERNAL[r])) % p)
        s = matvec_many(INTERNAL_MATRIX, s)
    for r in range(4, 8):
        s = matvec_many(EXTERNAL_MATRIX, sbox_many((s + np.array(RC_EXTERNAL[r], dtype=np.uint64)) % p))
    return s


def hash_felts(xs):
    s = [0] * 16
    for i in range(0, len(xs), 8):
        chunk = [int(x) % P for x in xs[i:i + 8]]
        s[:len(chunk)] = chunk                    # a short tail leaves the other rate lanes as the last permutation made them
        s = permute(s)
    return s[:8]


def compress(left, right):
    return permute(list(left) + list(right))[:8]


def merkle_commit(rows):
    """rows[i] = the concatenated row i of all tensors (canonical), len(rows) a power of two ->
    (tree: 2h - 1 digests, layers leaf-first back to back; root; commitment)."""
    h = len(rows)
    assert h and h & (h - 1) == 0
    tree = [hash_felts(r) for r in rows]
    off, n = 0, h
    while n > 1:
        tree += [compress(tree[off + 2 * i], tree[off + 2 * i + 1]) for i in range(n // 2)]
        off, n = off + n, n // 2
    root = tree[-1]
    return tree, root, compress(root, hash_felts([h.bit_length() - 1, len(rows[0])]))


def reverse_bits_len(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def rs_encode(column, log_blowup):
    """One column of n = 2^k canonical coefficients -> its N = n 2^log_blowup evaluations, bit-reversed: O(n N)."""
    n = len(column)
    assert n and n & (n - 1) == 0
    log_N = n.bit_length() - 1 + log_blowup
    N = 1 << log_N
    pw = [1] * N
    w = two_adic_generator(log_N)
    for i in range(1, N):
        pw[i] = pw[i - 1] * w % P
    out = [0] * N
    for k in range(N):
        out[reverse_bits_len(k, log_N)] = sum(int(c) * pw[k * i % N] for i, c in enumerate(column) if c) % P
    return out
