"""The BabyBear operations of sp1_amd/csrc/bb31.hpp at their edges, in both forms: the BB_HD code on the host and a gfx950
kernel with one lane per record (tests/native/bb31_ops.hip, which includes the header unchanged). Every result word is checked
against Python integers computed here from p and R = 2^32 alone; the linear layers, the S-box and the permutation come from
oracle/bb_py.py (canonical integers, explicit matrices, no Montgomery words). Nothing here is compared with bb31.hpp itself or
with oracle/bb_commit.hpp, which restates the header's formulation.

Kernels see stored (Montgomery) words, so the edges are chosen in that domain (tests/bb_edges.py). monty_reduce is called at
the ends of its documented domain and never outside. test_documented_bounds restates each range argument of the header's
comments as arithmetic, so that a comment which drifts from the code is noticed."""
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import bb_py
from bb_edges import EDGE_WORDS, P, R, R_INV, V16, canon, edge_states, permuted_edge_states, stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "bb31_ops.hip")
EXE = os.path.join(ROOT, "tests", "native", "bb31_ops")

M32 = R - 1
MU = 0x88000001
OP_NAMES = ["add", "sub", "mul", "monty_reduce", "to_monty", "pow", "two_adic_generator", "external_linear", "internal_linear",
            "sbox", "permute"]
OP_ADD, OP_SUB, OP_MUL, OP_REDUCE, OP_TO_MONTY, OP_POW, OP_GEN, OP_EXTERNAL, OP_INTERNAL, OP_SBOX, OP_PERMUTE = range(11)
STATE_OPS = (OP_EXTERNAL, OP_INTERNAL, OP_SBOX, OP_PERMUTE)

REDUCE_TOP = R * P                                  # monty_reduce: "x < 2^32 p" (exclusive)
INTERNAL_MAX = 16 * (P - 1) + ((P - 1) << 15)       # the largest argument internal_linear can pass


def test_documented_bounds():
    """Each range argument in bb31.hpp's comments, as arithmetic."""
    assert all(w < P for w in EDGE_WORDS)
    # the Montgomery constant: p MU = 1 mod 2^32
    assert P * MU % R == 1 and MU == pow(P, -1, R)
    # monty_reduce: u = t p with t < 2^32 is < 2^32 p, and both x and u fit 64 bits, so `x - u` wraps exactly when x < u
    assert M32 * P < REDUCE_TOP < 1 << 64
    # ... x = u mod 2^32, so (x - u) / 2^32 is an integer in (-p, p): `hi + P` of the wrapped difference is in [1, p), no overflow
    assert (REDUCE_TOP - 1) >> 32 < P and (M32 * P) >> 32 < P
    # add: a + b <= 2p - 2 fits 32 bits and one subtraction brings it under p; sub: a + p - b < 2p fits 32 bits
    assert 2 * (P - 1) < R and 2 * (P - 1) - P < P and (P - 1) + P < R
    # mul: a product of reduced words is inside the domain
    assert (P - 1) ** 2 < REDUCE_TOP
    # to_monty: (c mod p) (R^2 mod p) likewise
    assert (P - 1) * (R * R % P) < REDUCE_TOP
    # internal_linear: the 64-bit sum of sixteen words, the shift-add of lane 15 and the lane-0 form stay far inside it
    assert 16 * (P - 1) < 1 << 35 and INTERNAL_MAX < 1 << 47 < REDUCE_TOP
    assert 16 * (P - 1) - 0 + P < REDUCE_TOP          # sum - v0 + (p - v0) at its largest: v0 = 1 under fifteen p - 1, or less
    # ... and its shifts are the diagonal [-2, 1, 2, 4, ..., 2^13, 2^15]: lane i >= 1 shifts by i - 1, lane 15 by 15
    assert bb_py.INTERNAL_DIAG == [-2] + [1 << (15 if i == 15 else i - 1) for i in range(1, 16)]
    # two_adic_generator: p - 1 = 2^27 * 15
    assert (P - 1) >> 27 == 15 and (P - 1) % (1 << 27) == 0 and bb_py.TWO_ADICITY == 27


def test_bb_py_is_self_consistent():
    """The batched numpy form of the model equals its Python-integer form; the matrices are what their names say."""
    m4 = bb_py.M4
    assert m4 == [[2, 3, 1, 1], [1, 2, 3, 1], [1, 1, 2, 3], [3, 1, 1, 2]]
    for i in range(16):
        for j in range(16):
            assert bb_py.EXTERNAL_MATRIX[i][j] == (2 if i // 4 == j // 4 else 1) * m4[i % 4][j % 4]
            d = [P - 2, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 32768][i]
            assert bb_py.INTERNAL_MATRIX[i][j] == (1 + (d if i == j else 0)) * R_INV % P
    states = canon(edge_states()[:80])
    many = bb_py.permute_many(states)
    for s, want in zip(states.tolist(), many.tolist()):
        assert bb_py.permute(s) == want
    assert bb_py.permute([0] * 16) != [0] * 16


def reducer_inputs():
    """monty_reduce arguments, all inside [0, 2^32 p)."""
    rng = np.random.default_rng(3131)
    xs = [0, 1, 2, M32, R, R + 1, (P - 1) ** 2, REDUCE_TOP - 1, REDUCE_TOP - R, INTERNAL_MAX, INTERNAL_MAX - 1, 16 * (P - 1) + P,
          (P - 1) * (R * R % P)]
    xs += [k << 32 for k in (1, 2, 0xFFFF, 0x10000, P - 2, P - 1, V16)]                                  # zero low word
    xs += [(k << 32) | lo for k in (0, 1, P - 1, V16) for lo in (M32, 1, P, P - 1, V16, MU, 0x80000000)]
    xs += [a * b for a in EDGE_WORDS for b in EDGE_WORDS]
    xs += [int(v) % REDUCE_TOP for v in rng.integers(0, 1 << 64, 4096, dtype=np.uint64)]
    xs += [int(v) for v in rng.integers(0, 1 << 47, 2048, dtype=np.uint64)]                              # internal_linear's range
    return xs


@functools.lru_cache(maxsize=None)
def scalar_records():
    """[(op, n, x, a, b)] with every operand inside the operation's contract."""
    rng = np.random.default_rng(3100)
    recs = []
    pairs = [(a, b) for a in EDGE_WORDS for b in EDGE_WORDS]
    pairs += [(int(a), int(b)) for a, b in rng.integers(0, P, (1 << 16, 2))]
    for a, b in pairs:
        for op in (OP_ADD, OP_SUB, OP_MUL):
            recs.append((op, 0, 0, a, b))
    for c in [0, 1, P - 1, P, P + 1, M32] + EDGE_WORDS + [int(v) for v in rng.integers(0, 1 << 32, 1024)]:
        recs.append((OP_TO_MONTY, 0, 0, c, 0))
    for a in EDGE_WORDS + [int(v) for v in rng.integers(0, P, 64)]:
        for e in (0, 1, 2, 7, P - 1, P - 2, (P - 1) >> 27, (1 << 64) - 1, int(rng.integers(0, 1 << 63))):
            recs.append((OP_POW, 0, e, a, 0))
    for x in reducer_inputs():
        recs.append((OP_REDUCE, 0, x, 0, 0))
    for bits in range(bb_py.TWO_ADICITY + 1):
        recs.append((OP_GEN, bits, 0, 0, 0))
    return recs


def expected_scalar(rec):
    op, n, x, a, b = rec
    if op == OP_ADD:
        return (a + b) % P
    if op == OP_SUB:
        return (a - b) % P
    if op == OP_MUL:
        return a * b * R_INV % P
    if op == OP_REDUCE:
        return x * R_INV % P
    if op == OP_TO_MONTY:
        return a * R % P
    if op == OP_POW:
        return pow(a * R_INV % P, x, P) * R % P
    if op == OP_GEN:
        return bb_py.two_adic_generator(n) * R % P
    raise ValueError(op)


def check_scalar(rec, got):
    if got[1:] != [0] * 15 or got[0] != expected_scalar(rec):
        return False
    if rec[0] == OP_GEN:            # order exactly 2^bits
        g, n = got[0] * R_INV % P, rec[1]
        return pow(g, 1 << n, P) == 1 and (n == 0 or pow(g, 1 << (n - 1), P) != 1)
    return True


@functools.lru_cache(maxsize=None)
def expected_states():
    """{op: [n][16] stored words} for edge_states(): the linear layers act on stored words as they stand (they are linear, and
    the internal layer's 2^-32 is part of its matrix); the S-box and the permutation go through canonical values."""
    st = edge_states().astype(np.uint64)
    return {OP_EXTERNAL: bb_py.matvec_many(bb_py.EXTERNAL_MATRIX, st).astype(np.uint32),
            OP_INTERNAL: bb_py.matvec_many(bb_py.INTERNAL_MATRIX, st).astype(np.uint32),
            OP_SBOX: stored(bb_py.sbox_many(canon(edge_states()[:, 0]))),
            OP_PERMUTE: permuted_edge_states()}


def _encode():
    recs, states = scalar_records(), edge_states()
    words = np.zeros((len(recs) + len(STATE_OPS) * len(states), 20), np.uint32)
    n = len(recs)
    words[:n, 0] = [r[0] for r in recs]
    words[:n, 1] = [r[1] for r in recs]
    words[:n, 2] = [r[2] & M32 for r in recs]
    words[:n, 3] = [r[2] >> 32 for r in recs]
    words[:n, 4] = [r[3] for r in recs]
    words[:n, 5] = [r[4] for r in recs]
    for k, op in enumerate(STATE_OPS):
        rows = slice(n + k * len(states), n + (k + 1) * len(states))
        words[rows, 0] = op
        words[rows, 4:] = states
    return np.concatenate([np.array([len(words)], np.uint32), words.reshape(-1)])


def run_and_check(exe, form, timeout):
    recs, states = scalar_records(), edge_states()
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        _encode().tofile(fin)
        r = subprocess.run([exe, form, fin, fout], capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stdout + r.stderr
        out = np.fromfile(fout, dtype="<u4").reshape(-1, 16)
    n = len(recs)
    assert out.shape[0] == n + len(STATE_OPS) * len(states)
    bad = [(OP_NAMES[rec[0]], rec[1], hex(rec[2]), hex(rec[3]), hex(rec[4]), [hex(v) for v in got[:2]])
           for rec, got in zip(recs, out[:n].tolist()) if not check_scalar(rec, got)]
    assert not bad, "%s: %d of %d scalar records wrong, first: %s" % (form, len(bad), n, bad[:8])
    want = expected_states()
    for k, op in enumerate(STATE_OPS):
        got = out[n + k * len(states):n + (k + 1) * len(states)]
        if op == OP_SBOX:
            assert not got[:, 1:].any()
            got = got[:, 0]
        wrong = np.nonzero((got != want[op]).reshape(len(states), -1).any(axis=1))[0]
        assert wrong.size == 0, "%s: %s wrong on %d of %d states, first: state %d = %s -> %s, want %s" % (
            form, OP_NAMES[op], wrong.size, len(states), wrong[0], [hex(v) for v in states[wrong[0]]],
            [hex(v) for v in np.atleast_1d(got[wrong[0]])], [hex(v) for v in np.atleast_1d(want[op][wrong[0]])])
    return out.shape[0]


def test_operand_set_covers_the_edges():
    """The set itself: every operation appears, every operand is inside its function's domain, and the cases that sit on a
    bound or take the rarer branch are in it."""
    recs, states = scalar_records(), edge_states()
    assert {r[0] for r in recs} | set(STATE_OPS) == set(range(len(OP_NAMES)))
    by_op = lambda op: [r for r in recs if r[0] == op]
    for r in recs:
        if r[0] != OP_TO_MONTY:
            assert r[3] < P and r[4] < P, r
    assert int(states.max()) == P - 1 and states.shape[1] == 16
    xs = [r[2] for r in by_op(OP_REDUCE)]
    assert all(x < REDUCE_TOP for x in xs) and {0, 1, (P - 1) ** 2, REDUCE_TOP - 1, INTERNAL_MAX} <= set(xs)
    assert sum(1 for x in xs if x and x & M32 == 0) >= 7
    borrow = [x < ((x & M32) * MU & M32) * P for x in xs]             # x < u: the `hi + P` branch
    assert sum(borrow) > 1000 and len(borrow) - sum(borrow) > 1000
    adds = {(r[3], r[4]) for r in by_op(OP_ADD)}
    assert (1, P - 1) in adds and (P - 1, P - 1) in adds and ((P + 1) // 2, (P - 1) // 2) in adds      # s == p, the largest s
    subs = {(r[3], r[4]) for r in by_op(OP_SUB)}
    assert (0, P - 1) in subs and (P - 1, P - 1) in subs and (0, 0) in subs
    assert {0, 1, P - 1, P, P + 1, M32} <= {r[3] for r in by_op(OP_TO_MONTY)}
    assert {0, 1, P - 1, P - 2} <= {r[2] for r in by_op(OP_POW)}
    assert {r[1] for r in by_op(OP_GEN)} == set(range(28))
    rows = {tuple(s) for s in states[:60].tolist()}
    assert {(0,) * 16, (P - 1,) * 16, (V16,) * 16, (0,) + (P - 1,) * 15, (P - 1,) + (0,) * 15, (0, P - 1) * 8} <= rows
    assert all(tuple(P - 1 if i == lane else 0 for i in range(16)) in rows for lane in range(16))
    # internal_linear's largest argument is reached: sixteen lanes of p - 1, lane 15 shifted by 15
    assert 16 * (P - 1) + ((P - 1) << 15) == INTERNAL_MAX


def _host_compiler():
    gxx = shutil.which("g++")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if gxx is None or not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        return None, None
    return gxx, rocm


def test_host_form_matches_python():
    """bb31.hpp's BB_HD code compiled for the CPU by a plain C++ compiler: no GPU is opened."""
    gxx, rocm = _host_compiler()
    if gxx is None:
        pytest.skip("no g++ or no HIP headers")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bb31_ops_host")
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                               "-I" + os.path.join(ROOT, "sp1_amd", "csrc"), "-x", "c++", SRC, "-o", exe])
        assert run_and_check(exe, "host", timeout=300) > 1 << 17


@pytest.mark.gpu
def test_device_form_matches_python():
    assert os.path.exists(EXE), "tests/native/bb31_ops is not built (__graft_entry__.build())"
    assert run_and_check(EXE, "device", timeout=120) > 1 << 17
