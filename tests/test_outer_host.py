"""CPU checks of the outer (BN254) layer: the generated constants, the host permutation and the host MultiField32Challenger
against tests/outer_model.py (an independent restatement of the specification in Python ints), and argument validation of
the new entry points. Needs only libsp1hip.so; no device."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import outer_model as M  # noqa: E402

REFERENCE_RC = "/root/reference/slop/crates/bn254/src/poseidon2_rc.rs"
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_hip()
    from sp1_amd import _lib
    return _lib.load()


def _ptr(a):
    return a.ctypes.data_as(u32p)


def test_generator_output_is_the_committed_inc():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "sp1_amd", "gen_outer_constants.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_generator_and_model_agree_on_the_constants():
    sys.path.insert(0, os.path.join(ROOT, "sp1_amd"))
    import gen_outer_constants as G
    full, partial = G.round_constants()
    rc = M.round_constants()
    assert [tuple(r) for r in full[:4]] == rc[:4] and [tuple(r) for r in full[4:]] == rc[60:]
    assert partial == [r[0] for r in rc[4:60]]
    assert len(set(partial)) == 56


def test_model_reproduces_the_known_answer():
    assert M.permute(M.KNOWN_ANSWER_IN) == M.KNOWN_ANSWER_OUT


@pytest.mark.skipif(not os.path.exists(REFERENCE_RC), reason="reference tree not present")
def test_constants_equal_the_reference_table():
    text = open(REFERENCE_RC).read()
    block = text[text.index("RC3_HEX"):]
    block = block[block.index("["):]
    vals = [int(h, 16) for h in re.findall(r'"(0x[0-9a-fA-F]+)"', block)[:192]]
    rows = [tuple(vals[3 * i:3 * i + 3]) for i in range(64)]
    assert rows == M.round_constants()


def _host_permute(lib, states):
    """states: list of [a, b, c] canonical ints -> permuted canonical ints through the library's host permutation."""
    w = np.stack([np.concatenate([M.to_words(x) for x in s]) for s in states]).astype(np.uint32)
    assert lib.sp1hip_outer_poseidon2_permute_host(_ptr(w), len(states)) == 0
    return [[M.from_words(w[i, 8 * k:8 * k + 8]) for k in range(3)] for i in range(len(states))]


def test_host_permutation_known_answer(lib):
    assert _host_permute(lib, [M.KNOWN_ANSWER_IN]) == [M.KNOWN_ANSWER_OUT]


def test_host_permutation_matches_model_on_random_states(lib):
    rng = np.random.default_rng(11)
    states = [[int.from_bytes(rng.bytes(32), "little") % M.P for _ in range(3)] for _ in range(1000)]
    states[:4] = [[0, 0, 0], [M.P - 1] * 3, [1, 0, 0], [0, 0, M.P - 1]]
    assert _host_permute(lib, states) == [M.permute(s) for s in states]


def _gnark_kat():
    """The second published vector (tests/golden/outer_poseidon2_kat.json: SP1's gnark test of the permutation)."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "outer_poseidon2_kat.json")) as f:
        v = json.load(f)["vectors"]
    return [([int(x, 16) for x in t["input"]], [int(x, 16) for x in t["output"]]) for t in v]


def test_model_reproduces_the_gnark_known_answer():
    kats = _gnark_kat()
    assert [i for i, _ in kats] == [[0, 0, 0]]
    for i, o in kats:
        assert M.permute(i) == o


def test_host_permutation_gnark_known_answer(lib):
    kats = _gnark_kat()
    assert _host_permute(lib, [i for i, _ in kats]) == [o for _, o in kats]


class _Lib:
    """The host challenger through the raw C ABI (no torch, no device)."""

    def __init__(self, lib, h=None):
        self.lib = lib
        if h is None:
            h = C.c_void_p()
            assert lib.sp1hip_outer_challenger_new(C.byref(h)) == 0
        self.h = h

    def clone(self):
        out = C.c_void_p()
        assert self.lib.sp1hip_outer_challenger_clone(self.h, C.byref(out)) == 0
        return _Lib(self.lib, out)

    def observe_many(self, ms):
        a = np.asarray(ms, dtype=np.uint32)
        assert self.lib.sp1hip_outer_challenger_observe(self.h, _ptr(a), a.size) == 0

    def observe_commitment(self, x):
        a = M.to_words(x)
        a = np.asarray(a, dtype=np.uint32)
        assert self.lib.sp1hip_outer_challenger_observe_commitment(self.h, _ptr(a)) == 0

    def sample(self):
        v = C.c_uint32()
        assert self.lib.sp1hip_outer_challenger_sample(self.h, C.byref(v)) == 0
        return v.value

    def sample_ext(self):
        from sp1_amd._lib import Ext
        e = Ext()
        assert self.lib.sp1hip_outer_challenger_sample_ext(self.h, C.byref(e)) == 0
        return list(e.c)

    def sample_bits(self, bits):
        v = C.c_uint32()
        assert self.lib.sp1hip_outer_challenger_sample_bits(self.h, bits, C.byref(v)) == 0
        return v.value

    def check_witness(self, bits, w):
        ok = C.c_int()
        assert self.lib.sp1hip_outer_challenger_check_witness(self.h, bits, w, C.byref(ok)) == 0
        return bool(ok.value)

    def state(self):
        a = np.zeros(50, np.uint32)
        assert self.lib.sp1hip_outer_challenger_state(self.h, _ptr(a)) == 0
        return a

    def __del__(self):
        self.lib.sp1hip_outer_challenger_free(self.h)


def _kb(vals):
    return [M.kb_to_monty(v) for v in vals]


def test_challenger_grinding_prefix(lib):
    """observe 0..3 then sample (the prefix of the reference's grinding test)."""
    a, m = _Lib(lib), M.Challenger()
    a.observe_many(_kb(range(4)))
    m.observe_many(_kb(range(4)))
    assert np.array_equal(a.state(), m.state())
    assert a.sample() == m.sample()
    assert np.array_equal(a.state(), m.state())


@pytest.mark.parametrize("n", [15, 16, 17, 31, 32, 33])
def test_challenger_observe_counts(lib, n):
    a, m = _Lib(lib), M.Challenger()
    vals = _kb([(7919 * i + 3) % M.KB_P for i in range(n)])
    a.observe_many(vals)
    m.observe_many(vals)
    assert np.array_equal(a.state(), m.state())
    assert [a.sample() for _ in range(10)] == [m.sample() for _ in range(10)]      # crosses an output refill
    assert np.array_equal(a.state(), m.state())


def test_challenger_sample_after_sample_pops_without_duplex(lib):
    a, m = _Lib(lib), M.Challenger()
    a.observe_many(_kb([5]))
    m.observe_many(_kb([5]))
    a.sample()
    m.sample()
    before = a.state()
    assert before[41] == 7                                        # one popped of eight
    assert a.sample() == m.sample()
    after = a.state()
    assert np.array_equal(after[:24], before[:24]) and after[41] == 6
    assert np.array_equal(after, m.state())


def test_challenger_interleaved_script(lib):
    rng = np.random.default_rng(5)
    a, m = _Lib(lib), M.Challenger()
    for step in range(120):
        op = int(rng.integers(0, 5))
        if op == 0:
            vals = _kb(rng.integers(0, M.KB_P, int(rng.integers(1, 20))).tolist())
            a.observe_many(vals)
            m.observe_many(vals)
        elif op == 1:
            x = int.from_bytes(rng.bytes(32), "little") % M.P
            a.observe_commitment(x)
            m.observe_commitment(x)
        elif op == 2:
            assert a.sample_ext() == m.sample_ext()
        elif op == 3:
            bits = int(rng.integers(1, 31))
            assert a.sample_bits(bits) == m.sample_bits(bits)
        else:
            assert a.sample() == m.sample()
        assert np.array_equal(a.state(), m.state()), step


def test_challenger_check_witness_accepts_and_rejects(lib):
    base, mbase = _Lib(lib), M.Challenger()
    base.observe_many(_kb(range(1, 12)))
    mbase.observe_many(_kb(range(1, 12)))
    bits, seen = 4, {True: 0, False: 0}
    for w in range(64):
        a, m = base.clone(), mbase.clone()
        ok = a.check_witness(bits, M.kb_to_monty(w))
        assert ok == m.check_witness(bits, M.kb_to_monty(w))
        assert np.array_equal(a.state(), m.state())
        seen[ok] += 1
    assert seen[True] > 0 and seen[False] > 0


def test_bad_arguments_return_a_status(lib):
    from sp1_amd._lib import ERROR_INVALID_ARGUMENT as BAD, Tensor
    assert lib.sp1hip_outer_poseidon2_permute_host(None, 1) == BAD
    assert lib.sp1hip_outer_poseidon2_permute_host(None, 0) == 0
    bad = np.zeros(24, np.uint32)
    bad[:8] = 0xFFFFFFFF                                        # >= p: not a Montgomery word
    assert lib.sp1hip_outer_poseidon2_permute_host(_ptr(bad), 1) == BAD
    assert lib.sp1hip_outer_poseidon2_permute(None, 1, None) == BAD
    assert lib.sp1hip_outer_merkle_commit(None, 0, 3, None, None, None) == BAD
    t = (Tensor * 1)(Tensor(None, 0))
    dummy = np.zeros(64, np.uint32)
    assert lib.sp1hip_outer_merkle_commit(t, 1, 31, dummy.ctypes.data, dummy.ctypes.data, None) == BAD
    assert lib.sp1hip_outer_merkle_commit(t, 1, 3, dummy.ctypes.data, dummy.ctypes.data, None) == BAD       # width 0
    assert b"width 0" in lib.sp1hip_last_error()
    assert lib.sp1hip_outer_merkle_commit(t, 1, 3, None, dummy.ctypes.data, None) == BAD
    assert lib.sp1hip_outer_merkle_open(None, 0, 31, None, None, 1, None, None, None) == BAD
    assert lib.sp1hip_outer_commit_mles(None, 0, 3, 1, None, None, None, None) == BAD
    ptrs = (C.c_void_p * 1)(None)
    out8 = np.zeros(8, np.uint32)
    assert lib.sp1hip_outer_commit_mles(t, 1, 3, 1, ptrs, dummy.ctypes.data, _ptr(out8), None) == BAD
    assert lib.sp1hip_outer_commit_mles(t, 1, 30, 1, ptrs, dummy.ctypes.data, _ptr(out8), None) == BAD
    assert lib.sp1hip_outer_challenger_new(None) == BAD
    assert lib.sp1hip_outer_challenger_observe(None, None, 0) == BAD
    assert lib.sp1hip_outer_challenger_observe_commitment(None, None) == BAD
    assert lib.sp1hip_outer_challenger_grind(None, 4, None, None) == BAD
    h = C.c_void_p()
    assert lib.sp1hip_outer_challenger_new(C.byref(h)) == 0
    v = C.c_uint32()
    assert lib.sp1hip_outer_challenger_grind(h, 31, C.byref(v), None) == BAD
    assert lib.sp1hip_outer_challenger_grind(h, -1, C.byref(v), None) == BAD
    assert lib.sp1hip_outer_challenger_sample_bits(h, 32, C.byref(v)) == BAD
    assert lib.sp1hip_outer_challenger_check_witness(h, 4, M.KB_P, C.byref(C.c_int())) == BAD
    big = np.array([M.KB_P], np.uint32)
    assert lib.sp1hip_outer_challenger_observe(h, _ptr(big), 1) == BAD
    assert lib.sp1hip_outer_challenger_observe_commitment(h, _ptr(np.full(8, 0xFFFFFFFF, np.uint32))) == BAD
    st = np.zeros(50, np.uint32)
    assert lib.sp1hip_outer_challenger_state(h, _ptr(st)) == 0 and not st.any()   # nothing was accepted
    lib.sp1hip_outer_challenger_free(h)


def test_python_word_conversions():
    from sp1_amd import api
    for x in (0, 1, 2, M.P - 1, 12345678901234567890):
        w = api.outer_to_words(x)
        assert w.tolist() == M.to_words(x) and api.outer_from_words(w) == x
    assert api.outer_to_words(1).tolist() == M.to_words(1)
    assert api.outer_from_words(api.outer_to_words([3, 4])) == [3, 4]
