"""The two BabyBear references against each other, without a GPU: oracle/bb_py.py (canonical Python integers, the linear
layers as explicit matrices, the naive DFT; written from the definitions) and the C++ oracle (oracle/bb_commit.hpp, which
restates the kernels' Montgomery formulation). A formula both the kernel and the C++ oracle restate the same wrong way would
show here."""
import ctypes as C

import numpy as np
import pytest

import bb_py
import pyoracle as orc
from bb_edges import (P, R, RS_EDGE_LG_N, RS_EDGE_LOG_BLOWUPS, canon, edge_states, ntt_columns, permuted_edge_states, pool_tensor,
                      split_width, stored)


def test_field_constants():
    assert bb_py.P == P == orc.BB_P and bb_py.two_adic_generator(27) == 440564289        # the published generator of order 2^27
    lib = orc.lib()
    lib.orc_bb_two_adic_generator.restype = C.c_uint32
    for bits in range(28):
        g = bb_py.two_adic_generator(bits)
        assert g == lib.orc_bb_two_adic_generator(bits)
        assert pow(g, 1 << bits, P) == 1 and (bits == 0 or pow(g, 1 << (bits - 1), P) == P - 1)
    words = np.array([0, 1, P - 1, 0x0FFFFFFE], np.uint32)
    assert stored(canon(words)).tolist() == words.tolist() and canon(words).tolist() == [0, pow(R, -1, P), (P - 1) * pow(R, -1, P) % P, 1]


def test_permutation_of_edge_states_matches_the_oracle():
    assert np.array_equal(orc.bb_permute(edge_states()), permuted_edge_states())


@pytest.mark.parametrize("lg_n", range(0, 7))
def test_naive_dft_matches_the_oracle_rs_encode(lg_n):
    m = ntt_columns(lg_n)
    cm = canon(m)
    for lb in (0, 1, 2):
        want = orc.bb_rs_encode(m, lb)
        for c in range(m.shape[1]):
            assert stored(bb_py.rs_encode(cm[:, c].tolist(), lb)).tolist() == want[:, c].tolist(), (lg_n, lb, c)


@pytest.mark.parametrize("height", [1, 2, 8])
def test_merkle_commit_matches_the_oracle(height):
    """Sponge tails at every residue around the rate, tensor boundaries inside a rate block, the metadata hash."""
    for width in (0, 1, 7, 8, 9, 15, 16, 17, 30):
        for fill in (P - 1, None):
            ts = [np.full((height, w), fill, np.uint32) if fill is not None else pool_tensor((height, w), 100 * width + k)
                  for k, w in enumerate(split_width(width))]
            tree, root, commit = orc.bb_merkle_commit(ts)
            py_tree, py_root, py_commit = bb_py.merkle_commit(canon(np.concatenate(ts, axis=1)).tolist())
            assert stored(py_tree).tolist() == tree.tolist(), (width, fill)
            assert stored(py_root).tolist() == root.tolist() and stored(py_commit).tolist() == commit.tolist()


def test_commit_mles_is_encode_then_merkle_commit():
    """orc.bb_commit_mles (the reference of tests/test_gpu_babybear.py) is the composition of the two pieces tested above."""
    ms = [pool_tensor((8, 5), 1), pool_tensor((8, 3), 2)]
    commit, cws, tree = orc.bb_commit_mles(ms, 1, True, True)
    enc = [orc.bb_rs_encode(m, 1) for m in ms]
    assert all(np.array_equal(a, b) for a, b in zip(cws, enc))
    t2, _, c2 = orc.bb_merkle_commit(enc)
    assert np.array_equal(t2, tree) and np.array_equal(c2, commit)


def _pass_plan(log_N):
    """[(b, l)] per pass, restated from rs_encode in babybear.hip: b = s_hi % 8 ?: 8 stages, tile width l = min(low_bits, 12 - b)."""
    passes, s_hi = [], log_N
    while s_hi >= 1:
        b = s_hi % 8 or 8
        passes.append((b, min(s_hi - b, 12 - b)))
        s_hi -= b
    return passes


def test_pass_plan_of_the_rs_encode_sizes():
    """The sizes of tests/test_gpu_bb_edges.py against the plan. low_bits is a multiple of 8, so l is 0 (low_bits = 0), 8 down to
    4 (low_bits = 8, b = 1..8) or 12 - b = 11 down to 4 (low_bits >= 16): 1, 2 and 3 are never reached at any size, 9 needs
    b = 3 over 16 low bits, which is log N = 19 first."""
    every = {l for log_N in range(0, 28) for _, l in _pass_plan(log_N)}
    assert every == {0} | set(range(4, 12))
    sizes = sorted({lg_n + lb for lg_n in RS_EDGE_LG_N for lb in RS_EDGE_LOG_BLOWUPS})
    assert sizes == list(range(0, 20))
    plans = [_pass_plan(log_N) for log_N in sizes]
    assert {v[0][0] for v in plans if v} == set(range(1, 9))          # every first-pass length
    assert {l for v in plans for _, l in v} == every                  # every tile width there is
    assert {len(v) for v in plans} == {0, 1, 2, 3}
    assert [b for b, _ in _pass_plan(24)] == [8, 8, 8] and [b for b, _ in _pass_plan(25)] == [1, 8, 8, 8]      # the at-size test
    # the twiddle walk of 16 entries per lane is cut short (half < 16) exactly for log N <= 4
    assert [log_N for log_N in sizes if (1 << max(log_N - 1, 0)) < 16] == [0, 1, 2, 3, 4]


def test_refusals_return_before_any_device_call():
    """Every refusal that tests/test_gpu_bb_edges.py makes with real buffers, here without a GPU and with pointers that are never
    dereferenced: each SP1HIP_REQUIRE of the three BabyBear entry points (and of make_tensor_table) answers before the first
    HIP call, which is what makes the refusal tests safe to run on a card."""
    from sp1_amd import _lib
    L = _lib.load()
    vp = lambda x: C.c_void_p(x) if x else None
    A, B = 0x10000, 0x20000
    for o, i, lg_n, lb, n in [(A, B, 27, 1, 1), (A, B, 28, 0, 1), (A, B, 0, 28, 1), (A, B, -1, 2, 1), (A, B, 2, -1, 1), (A, A, 2, 1, 1),
                              (A, B, 0, 0, 65536), (0, B, 2, 1, 1), (A, 0, 2, 1, 1)]:
        assert L.sp1hip_bb_rs_encode_batch(vp(o), vp(i), lg_n, lb, n, None) != 0 and b"rs_encode" in L.sp1hip_last_error()
    assert L.sp1hip_bb_rs_encode_batch(vp(A), vp(B), 2, 1, 0, None) == 0
    t = _lib.Tensor(C.c_void_p(B), 2)
    one, many, null_data = (_lib.Tensor * 1)(t), (_lib.Tensor * 257)(*[t] * 257), (_lib.Tensor * 1)(_lib.Tensor(None, 2))
    for arr, n, lg_h, tree, out in [(one, 1, 31, A, B), (one, 1, -1, A, B), (one, 1, 2, 0, B), (one, 1, 2, A, 0), (None, 1, 2, A, B),
                                    (one, 0, 2, A, B), (many, 257, 2, A, B), (null_data, 1, 2, A, B)]:
        assert L.sp1hip_bb_merkle_commit(arr, n, lg_h, vp(tree), vp(out), None) != 0
    ptrs, null_ptrs = (C.c_void_p * 1)(A), (C.c_void_p * 1)(None)
    commit = np.zeros(8, np.uint32)
    hc = commit.ctypes.data_as(_lib.u32p)
    for a, n, p, tree, h in [(one, 0, ptrs, A, hc), (None, 1, ptrs, A, hc), (one, 1, None, A, hc), (one, 1, null_ptrs, A, hc),
                             (one, 1, ptrs, 0, hc), (one, 1, ptrs, A, None)]:
        assert L.sp1hip_bb_commit_mles(a, n, 2, 1, p, vp(tree), h, None) != 0 and b"sp1hip_bb_commit_mles" in L.sp1hip_last_error()
    assert not commit.any()
    assert L.sp1hip_bb_poseidon2_permute(None, 0, None) == 0 and L.sp1hip_bb_poseidon2_permute(None, 1, None) != 0
