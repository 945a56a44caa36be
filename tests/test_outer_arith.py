"""The BN254 field operations of sp1_amd/csrc/bn254.hpp at their edges, in all three forms: the BN_HD code on the host, and
the device kernel with the Montgomery product as MulForm::Mad and as MulForm::LoHi (tests/native/bn254_ops.hip, which
includes the header unchanged). Every result is checked against Python integers computed here from p and R = 2^256 alone
(no library code, no tests/outer_model.py).

The operands are the values where this kind of code breaks: sums landing exactly on p, 2p, 4p and 5p - 5 (cond_sub at
x == m, the lazy reducers), limb products whose low word is 0 (the carry tests of the LoHi multiply-accumulate), the largest
packed reduce_31 value, all pairs of those, and 2^16 random and limb-structured pairs."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "bn254_ops.hip")
EXE = os.path.join(ROOT, "tests", "native", "bn254_ops")

P = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
R = 1 << 256
R_INV = pow(R, -1, P)
M256 = R - 1
KB_P = 0x7F000001

(OP_MUL, OP_SQR, OP_ADD, OP_DBL, OP_SUB, OP_TO_MONTY, OP_FROM_MONTY, OP_ADD_LAZY, OP_REDUCE_2P, OP_REDUCE_4P, OP_REDUCE_5P,
 OP_COND_SUB, OP_CMP, OP_PACK31) = range(14)
OP_NAMES = ["mul", "sqr", "add", "dbl", "sub", "to_monty", "from_monty", "add_lazy", "reduce_2p", "reduce_4p", "reduce_5p",
            "cond_sub", "cmp", "pack31"]


def _limbs(x):
    return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def _int(limbs):
    return sum(int(v) << (32 * i) for i, v in enumerate(limbs))


def edge_values():
    """Canonical values (< p) at the edges, and raw 256-bit words (any value) for the operations that take them."""
    canon = {0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, R % P, R * R % P, P - R % P}
    for k in list(range(32, 254, 32)) + [253]:
        canon |= {1 << k, (1 << k) - 1}
    raw = set(canon) | {P, P + 1, 2 * P, 4 * P, M256}
    for i in range(8):
        one_limb = 0xFFFFFFFF << (32 * i)                       # zero with one limb all-ones
        raw |= {one_limb, M256 ^ one_limb, 1 << (32 * i)}       # ... and all-ones with one limb zero
        canon |= {v for v in (one_limb, M256 ^ one_limb, 1 << (32 * i), (1 << (32 * i + 31))) if v < P}
    canon |= {_int(_limbs(P)[:7] + [0]), _int([0] * 7 + [_limbs(P)[7]]), P - (1 << 224)}
    return sorted(canon), sorted(raw)


def structured_values(rng, n):
    """Canonical values whose limbs come from {0, 1, 2^31, 2^32 - 1, 2^16 odd, random}: many limb products have a low word
    of 0 (the LoHi carry tests `s < t` with s == t) or carry out of every add."""
    pool = np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0x10000, 0xFFFF0000, 0x7F000000], dtype=np.uint64)
    pick = rng.integers(0, len(pool) + 2, (n, 8))
    rand = rng.integers(0, 1 << 32, (n, 8), dtype=np.uint64)
    odd16 = (rng.integers(0, 1 << 16, (n, 8), dtype=np.uint64) | 1) << 16
    limbs = np.where(pick < len(pool), pool[np.minimum(pick, len(pool) - 1)], np.where(pick == len(pool), rand, odd16))
    return [_int(row) % P for row in limbs.tolist()]


def random_values(rng, n, bound=P):
    return [int.from_bytes(rng.bytes(40), "little") % bound for _ in range(n)]


def expected(op, a, b):
    if op == OP_MUL:
        return a * b * R_INV % P
    if op == OP_SQR:
        return a * a * R_INV % P
    if op == OP_ADD:
        return (a + b) % P
    if op == OP_DBL:
        return 2 * a % P
    if op == OP_SUB:
        return (a - b) % P
    if op == OP_TO_MONTY:
        return a * R % P
    if op == OP_FROM_MONTY:
        return a * R_INV % P
    if op == OP_ADD_LAZY:
        return (a + b) & M256
    if op in (OP_REDUCE_2P, OP_REDUCE_4P, OP_REDUCE_5P):
        return a % P
    if op == OP_COND_SUB:
        return a - b if a >= b else a
    if op == OP_CMP:
        return ((a > b) - (a < b)) & 0xFFFFFFFF
    if op == OP_PACK31:
        return sum(v << (31 * i) for i, v in enumerate(_limbs(a)))
    raise ValueError(op)


def operand_set():
    """[(op, a, b)] with every operand inside the operation's contract."""
    rng = np.random.default_rng(2540)
    canon, raw = edge_values()
    recs = []
    # all pairs of edge values
    for a in canon:
        for op in (OP_SQR, OP_DBL, OP_TO_MONTY, OP_FROM_MONTY):
            recs.append((op, a, 0))
        for b in canon:
            for op in (OP_MUL, OP_ADD, OP_SUB):
                recs.append((op, a, b))
    for a in raw:
        for b in raw:
            for op in (OP_ADD_LAZY, OP_COND_SUB, OP_CMP):
                recs.append((op, a, b))
    # the lazy reducers at k p - 1, k p, k p + 1 (k = 1, 2, 4) and at 5p - 5 (2 x2 + s of lanes at p - 1), inside each domain
    lazy = sorted({v for k in (1, 2, 4) for v in (k * P - 1, k * P, k * P + 1)} | {0, 5 * P - 5, 5 * P - 1, 3 * P, 3 * P - 1})
    for op, top in ((OP_REDUCE_2P, 2 * P), (OP_REDUCE_4P, 4 * P), (OP_REDUCE_5P, 5 * P)):
        recs += [(op, x, 0) for x in lazy if x < top]
        recs += [(op, x, 0) for x in random_values(rng, 512, top)]
    for m in (P, 2 * P, 4 * P):
        recs += [(OP_COND_SUB, x, m) for x in (m - 1, m, m + 1, 2 * m - 1, 0, M256) if x <= M256]
    # pack31: every position holding p_KB - 1, 0 or 1 (and the largest 31-bit value) for n = 1 .. 8 used columns
    for n in range(1, 9):
        for fill in (KB_P - 1, 0, 1, (1 << 31) - 1):
            recs.append((OP_PACK31, _int([fill] * n + [0] * (8 - n)), 0))
            for i in range(n):
                for other in (0, KB_P - 1):
                    v = [other] * n + [0] * (8 - n)
                    v[i] = fill
                    recs.append((OP_PACK31, _int(v), 0))
    pk = rng.integers(0, KB_P, (256, 8), dtype=np.uint64).tolist()
    recs += [(OP_PACK31, _int(v), 0) for v in pk]
    # 2^16 random pairs (half uniform, half limb-structured) through the operations on canonical values
    n = 1 << 14
    for xs, ys in ((random_values(rng, n), random_values(rng, n)), (structured_values(rng, n), structured_values(rng, n))):
        for a, b in zip(xs, ys):
            recs += [(OP_MUL, a, b), (OP_ADD, a, b), (OP_SUB, a, b), (OP_CMP, a, b)]
        recs += [(OP_SQR, a, 0) for a in xs] + [(OP_TO_MONTY, a, 0) for a in ys] + [(OP_FROM_MONTY, a, 0) for a in xs]
    recs += [(OP_ADD_LAZY, a, b) for a, b in zip(random_values(rng, 4096, R), random_values(rng, 4096, R))]
    recs += [(OP_COND_SUB, a, b) for a, b in zip(random_values(rng, 4096, 5 * P), random_values(rng, 4096, 5 * P))]
    return recs


def _encode(recs):
    words = np.zeros((len(recs), 17), np.uint32)
    words[:, 0] = [r[0] for r in recs]
    blob = b"".join(r[1].to_bytes(32, "little") + r[2].to_bytes(32, "little") for r in recs)
    words[:, 1:] = np.frombuffer(blob, dtype="<u4").reshape(len(recs), 16)
    return np.concatenate([np.array([len(recs)], np.uint32), words.reshape(-1)])


def run_and_check(exe, form, timeout):
    recs = operand_set()
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        _encode(recs).tofile(fin)
        r = subprocess.run([exe, form, fin, fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout + r.stderr
        out = np.fromfile(fout, dtype="<u4").reshape(-1, 8)
    assert out.shape[0] == len(recs)
    got = [int.from_bytes(row.tobytes(), "little") for row in out]
    bad = [(OP_NAMES[op], hex(a), hex(b), hex(g), hex(expected(op, a, b)))
           for (op, a, b), g in zip(recs, got) if g != expected(op, a, b)]
    assert not bad, "%s: %d of %d wrong, first: %s" % (form, len(bad), len(recs), bad[:8])
    return len(recs)


def test_operand_set_covers_the_edges():
    """The set itself: every operation appears, and the sums that must land exactly on p, 2p, 4p and 5p - 5 are in it."""
    recs = operand_set()
    assert {r[0] for r in recs} == set(range(14))
    assert (OP_ADD, 1, P - 1) in recs and (OP_SUB, P - 1, P - 1) in recs
    assert (OP_COND_SUB, P, P) in recs
    for op, x in ((OP_REDUCE_5P, 5 * P - 5), (OP_REDUCE_5P, 4 * P), (OP_REDUCE_4P, 2 * P), (OP_REDUCE_2P, P)):
        assert (op, x, 0) in recs
    assert (OP_PACK31, _int([KB_P - 1] * 8), 0) in recs
    assert expected(OP_PACK31, _int([KB_P - 1] * 8), 0) < P
    # a limb product with a low word of 0 and a nonzero high word: 2^16 odd x 2^16 odd
    assert any(r[0] == OP_MUL and any(l % (1 << 16) == 0 and l for l in _limbs(r[1])) for r in recs)
    assert all(r[1] < P and r[2] < P for r in recs if r[0] in (OP_MUL, OP_SQR, OP_ADD, OP_DBL, OP_SUB, OP_TO_MONTY, OP_FROM_MONTY))


def _host_compiler():
    gxx = shutil.which("g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if gxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        return None, None
    return gxx, rocm


def test_host_form_matches_python():
    """bn254.hpp's BN_HD code compiled for the CPU by a plain C++ compiler: no GPU is opened."""
    gxx, rocm = _host_compiler()
    if gxx is None:
        pytest.skip("no g++ or no HIP headers")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bn254_ops_host")
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                               "-I" + os.path.join(ROOT, "sp1_amd", "csrc"), "-x", "c++", SRC, "-o", exe])
        assert run_and_check(exe, "host", timeout=300) > 1 << 16


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["mad", "lohi"])
def test_device_forms_match_python(form):
    assert os.path.exists(EXE), "tests/native/bn254_ops is not built (__graft_entry__.build())"
    assert run_and_check(EXE, form, timeout=120) > 1 << 16
