"""Edge-valued inputs (-m gpu) through the C ABI of the BabyBear commit path (sp1_amd/csrc/babybear.hip): every exported entry
point, every refusal of their argument checks, the NTT pass plan at every transform size 2^0 .. 2^19 and at the three- and
four-pass sizes 2^24 and 2^25, trees of height 1 and over tensors that are not codewords, sponge tails at every residue that
matters. Words are chosen in the stored (Montgomery) domain (tests/bb_edges.py). Two references: the C++ oracle
(oracle/bb_commit.hpp, which restates the kernels' formulation) and oracle/bb_py.py (canonical Python integers, explicit
matrices, the naive DFT), tied together on the small shapes; closed forms (the encoding of a delta column is the powers of a
root of unity) where neither is affordable. Every comparison is exact.

The refusal tests exercise host-side argument checks that return before any launch (babybear.hip: rs_encode, merkle_commit,
sp1hip_bb_commit_mles; merkle.hip: make_tensor_table)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bb_py  # noqa: E402
import pyoracle as orc  # noqa: E402
from bb_edges import (P, R1, RS_EDGE_LG_N, RS_EDGE_LOG_BLOWUPS, V16, canon, edge_states, ntt_columns,  # noqa: E402
                      permuted_edge_states, pool_tensor, split_width, stored)

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


# ------------------------------------------------------------------ sp1hip_bb_rs_encode_batch

@pytest.mark.parametrize("lg_n", RS_EDGE_LG_N)
def test_rs_encode_of_edge_columns_matches_oracle(api, lg_n):
    """log N = lg_n + log_blowup reaches every value 0..19: tests/test_bb_py.py::test_pass_plan_of_the_rs_encode_sizes restates
    the pass plan and holds that every first-pass length and every reachable tile width is among them."""
    m = ntt_columns(lg_n)
    d_m = api.ColMajor.from_row_major_host(m)
    for lb in RS_EDGE_LOG_BLOWUPS:
        want = orc.bb_rs_encode(m, lb)
        got = api.bb_rs_encode_batch(d_m, lb).to_row_major_host()
        assert np.array_equal(got, want), (lg_n, lb)
        if lg_n <= 6:           # the naive DFT in Python integers: ties bb_py to the C++ oracle
            cm = canon(m)
            for c in range(m.shape[1]):
                assert stored(bb_py.rs_encode(cm[:, c].tolist(), lb)).tolist() == want[:, c].tolist(), (lg_n, lb, c)


def _bit_reverse_indices(bits, device):
    rev = torch.zeros(1, dtype=torch.int64, device=device)
    for _ in range(bits):
        rev = torch.cat([2 * rev, 2 * rev + 1])
    return rev


def _delta_codeword(lg_n, lb, index, word, device):
    """The encoding of the column with stored `word` at row `index` and 0 elsewhere: natural-order entry k is
    word * w^(k * index) with w = two_adic_generator(lg_n + lb) (a canonical power, so the product stays a stored word); the
    output rows are bit-reversed. Powers by doubling in int64 (every product is < 2^62)."""
    lg_t = lg_n + lb
    step = pow(bb_py.two_adic_generator(lg_t), index, P)
    pw = torch.ones(1, dtype=torch.int64, device=device)
    while pw.numel() < 1 << lg_t:
        pw = torch.cat([pw, pw * step % P])
        step = step * step % P
    return (pw * word % P)[_bit_reverse_indices(lg_t, device)].to(torch.int32)


@pytest.mark.parametrize("lg_n,lb", [(22, 2), (24, 1)])
def test_rs_encode_closed_forms_at_size(api, lg_n, lb):
    """Three passes (8 + 8 + 8) at 2^24 points and the four-pass plan (1 + 8 + 8 + 8) at 2^25. The closed form's convention
    (which root, which row order) is first established against the oracle at 2^3, 2^8 and 2^13 rows, then used at size: every
    row of the delta columns. For the constant and alternating columns row 0 is the column sum and row 1 the alternating sum
    (the DFT is linear in stored words)."""
    for small in (3, 8, 13):
        for index, word in ((0, P - 1), ((1 << small) - 1, V16), (5, R1)):
            col = np.zeros((1 << small, 1), np.uint32)
            col[index, 0] = word
            got = _delta_codeword(small, lb, index, word, "cpu").numpy().view(np.uint32)
            assert np.array_equal(orc.bb_rs_encode(col, lb)[:, 0], got), (small, index)
    n = 1 << lg_n
    deltas = [(0, P - 1), (n - 1, P - 1), (n // 2, V16), (n // 3, R1)]
    m = torch.zeros((len(deltas) + 3, n), dtype=torch.int32, device="cuda")           # column-major: [col][row]
    for c, (index, word) in enumerate(deltas):
        m[c, index] = word
    c0 = len(deltas)
    m[c0] = P - 1                                                                      # all p - 1
    m[c0 + 1, 1::2] = P - 1                                                            # 0 / p - 1 at stride 1
    m[c0 + 2].view(-1, 2 << (lg_n // 2))[:, :(1 << (lg_n // 2))] = P - 1              # p - 1 / 0 at stride 2^(lg_n / 2)
    out = api.bb_rs_encode_batch(api.ColMajor(m.reshape(-1), n, m.shape[0]), lb).words.view(m.shape[0], n << lb)
    for c, (index, word) in enumerate(deltas):
        assert torch.equal(out[c], _delta_codeword(lg_n, lb, index, word, "cuda")), (lg_n, index)
    cols = m[c0:].to(torch.int64)
    total = cols.sum(dim=1) % P
    alt = (cols[:, 0::2].sum(dim=1) - cols[:, 1::2].sum(dim=1)) % P
    head = out[c0:, :2].to(torch.int64)
    assert head[:, 0].tolist() == total.tolist() and head[:, 1].tolist() == alt.tolist()


def test_rs_encode_refusals_leave_the_output_untouched(api):
    """Every SP1HIP_REQUIRE of rs_encode, each of which returns before the first launch."""
    L, s = api._L(), api._stream_ptr()
    d_in = torch.full((16,), P - 1, dtype=torch.int32, device="cuda")
    out = torch.full((64,), SENTINEL, dtype=torch.int32, device="cuda")
    calls = [(out, d_in, 27, 1, 1), (out, d_in, 28, 0, 1), (out, d_in, 0, 28, 1),          # log_N = 28
             (out, d_in, -1, 2, 1), (out, d_in, 2, -1, 1), (out, d_in, -1, -1, 1),         # negative sizes
             (out, out, 2, 1, 1),                                                          # in place
             (out, d_in, 0, 0, 65536),                                                     # gridDim.y
             (None, d_in, 2, 1, 1), (out, None, 2, 1, 1)]
    for o, i, lg_n, lb, n_cols in calls:
        st = L.sp1hip_bb_rs_encode_batch(api._dptr(o) if o is not None else None, api._dptr(i) if i is not None else None,
                                         lg_n, lb, n_cols, s)
        assert st != 0 and b"rs_encode" in L.sp1hip_last_error(), (lg_n, lb, n_cols)
    assert L.sp1hip_bb_rs_encode_batch(api._dptr(out), api._dptr(d_in), 2, 1, 0, s) == 0    # no columns: success, nothing done
    assert L.sp1hip_bb_rs_encode_batch(None, None, 2, 1, 0, s) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((d_in == P - 1).all())


def test_rs_encode_of_65535_columns(api):
    """The largest accepted column count (one column per gridDim.y), 1 row, log_blowup 1: each output pair is (x, x)."""
    col = pool_tensor((1, 65535), 65535)
    col[0, :4] = [0, P - 1, V16, R1]
    got = api.bb_rs_encode_batch(api.ColMajor.from_row_major_host(col), 1).to_row_major_host()
    assert np.array_equal(got, np.concatenate([col, col]))


# ------------------------------------------------------------------ sp1hip_bb_merkle_commit

def _merkle_case(api, tensors):
    want_tree, want_root, want_commit = orc.bb_merkle_commit(tensors)
    commit, root, tree = api.bb_merkle_commit([api.ColMajor.from_row_major_host(t) for t in tensors])
    h = tensors[0].shape[0]
    assert np.array_equal(api.to_host(tree, (2 * h - 1, 8)), want_tree)
    assert np.array_equal(root, want_root) and np.array_equal(commit, want_commit)
    if h <= 8:                  # the sponge's tail rule and the metadata hash against the model that shares no code with the oracle
        rows = canon(np.concatenate(tensors, axis=1)).tolist()
        py_tree, py_root, py_commit = bb_py.merkle_commit(rows)
        assert stored(py_tree).tolist() == want_tree.tolist()
        assert stored(py_root).tolist() == root.tolist() and stored(py_commit).tolist() == commit.tolist()


@pytest.mark.parametrize("height", [1, 2, 8, 256, 512, 1 << 12])
def test_merkle_commit_of_raw_tensors(api, height):
    """Whole tree (2h - 1 digests), root and commitment over tensors that are not codewords: total widths around the rate,
    split so that a tensor boundary falls inside a rate block; constant tensors of 0, p - 1, 0x77ffffff and pool-drawn ones.
    Height 1 has no compress layer; 512 is the next legal height above 257 (two leaf workgroups, the second full)."""
    for width in (1, 7, 8, 9, 15, 16, 17, 200):
        assert sum(split_width(width)) == width
        for fill in (0, P - 1, V16, None):
            ts = [np.full((height, w), fill, np.uint32) if fill is not None else pool_tensor((height, w), 1000 * width + w + k)
                  for k, w in enumerate(split_width(width))]
            _merkle_case(api, ts)


def test_merkle_commit_of_64_tensors_of_width_1(api):
    _merkle_case(api, [pool_tensor((256, 1), 6400 + k) for k in range(64)])
    _merkle_case(api, [pool_tensor((4, 1), 6500 + k) for k in range(64)])


def test_merkle_commit_of_total_width_0_matches_oracle(api):
    """make_tensor_table accepts a message of empty tensors (null data is allowed at width 0): every leaf is the untouched zero
    state's first eight lanes, and the commitment hashes [lg_h, 0]."""
    L, s = api._L(), api._stream_ptr()
    h = 4
    arr = (api.Tensor * 2)(api.Tensor(None, 0), api.Tensor(None, 0))
    tree, rc = api.device_words((2 * h - 1) * 8), api.device_words(16)
    api.check(L.sp1hip_bb_merkle_commit(arr, 2, 2, api._dptr(tree), api._dptr(rc), s))
    want_tree, want_root, want_commit = orc.bb_merkle_commit([np.zeros((h, 0), np.uint32)] * 2)
    assert not want_tree[:h].any()
    assert np.array_equal(api.to_host(tree, (2 * h - 1, 8)), want_tree)
    assert np.array_equal(api.to_host(rc), np.concatenate([want_root, want_commit]))
    py_tree, _, py_commit = bb_py.merkle_commit([[]] * h)
    assert stored(py_tree).tolist() == want_tree.tolist() and stored(py_commit).tolist() == want_commit.tolist()


def test_merkle_commit_refusals_leave_the_outputs_untouched(api):
    """merkle_commit's SP1HIP_REQUIRE and make_tensor_table's, all before the first launch."""
    L, s = api._L(), api._stream_ptr()
    t = api.ColMajor(torch.full((8,), P - 1, dtype=torch.int32, device="cuda"), 4, 2)
    one = api._tensor_array([t])
    tree = torch.full((7 * 8,), SENTINEL, dtype=torch.int32, device="cuda")
    rc = torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda")
    many = (api.Tensor * 257)(*[t.as_tensor_struct()] * 257)
    null_data = (api.Tensor * 1)(api.Tensor(None, 2))
    calls = [(one, 1, 31, tree, rc), (one, 1, -1, tree, rc), (one, 1, 2, None, rc), (one, 1, 2, tree, None),
             (None, 1, 2, tree, rc), (one, 0, 2, tree, rc), (many, 257, 2, tree, rc), (null_data, 1, 2, tree, rc)]
    for arr, n, lg_h, tr, out in calls:
        st = L.sp1hip_bb_merkle_commit(arr, n, lg_h, api._dptr(tr) if tr is not None else None,
                                       api._dptr(out) if out is not None else None, s)
        assert st != 0, (n, lg_h)
    torch.cuda.synchronize()
    assert bool((tree == SENTINEL).all()) and bool((rc == SENTINEL).all())


# ------------------------------------------------------------------ sp1hip_bb_commit_mles

@pytest.mark.parametrize("lg_n,lb", [(0, 0), (0, 1), (3, 1), (10, 2)])
def test_commit_mles_of_edge_tensors(api, lg_n, lb):
    """Commitment, codewords and tree; (0, 0) is a height-one tree with no transform."""
    n = 1 << lg_n
    for fill in (0, P - 1, V16, None):
        ms = [np.full((n, w), fill, np.uint32) if fill is not None else pool_tensor((n, w), 77 * lg_n + w) for w in (5, 3, 9)]
        want_c, want_cw, want_tree = orc.bb_commit_mles(ms, lb, True, True)
        commit, cws, tree = api.bb_commit_mles([api.ColMajor.from_row_major_host(m) for m in ms], lb)
        assert np.array_equal(commit, want_c), fill
        for k in range(len(ms)):
            assert np.array_equal(cws[k].to_row_major_host(), want_cw[k]), (fill, k)
        assert np.array_equal(api.to_host(tree, want_tree.shape), want_tree), fill
        if lg_n + lb <= 3:
            _, _, py_commit = bb_py.merkle_commit(canon(np.concatenate(want_cw, axis=1)).tolist())
            assert stored(py_commit).tolist() == commit.tolist()


def test_commit_mles_refusals(api):
    L, s = api._L(), api._stream_ptr()
    m = api.ColMajor(torch.full((8,), P - 1, dtype=torch.int32, device="cuda"), 4, 2)
    arr = api._tensor_array([m])
    cw = torch.full((16,), SENTINEL, dtype=torch.int32, device="cuda")
    tree = torch.full((15 * 8,), SENTINEL, dtype=torch.int32, device="cuda")
    commit = np.full(8, SENTINEL, np.uint32)
    h_commit = commit.ctypes.data_as(api._lib.u32p)
    ptrs = (C.c_void_p * 1)(cw.data_ptr())
    null_ptrs = (C.c_void_p * 1)(None)
    calls = [(arr, 0, ptrs, tree, h_commit), (arr, -1, ptrs, tree, h_commit), (None, 1, ptrs, tree, h_commit),
             (arr, 1, None, tree, h_commit), (arr, 1, null_ptrs, tree, h_commit), (arr, 1, ptrs, None, h_commit),
             (arr, 1, ptrs, tree, None)]
    for a, n, p, tr, hc in calls:
        st = L.sp1hip_bb_commit_mles(a, n, 2, 1, p, api._dptr(tr) if tr is not None else None, hc, s)
        assert st != 0 and b"sp1hip_bb_commit_mles" in L.sp1hip_last_error(), n
    torch.cuda.synchronize()
    assert bool((cw == SENTINEL).all()) and bool((tree == SENTINEL).all()) and bool((commit == SENTINEL).all())


# ------------------------------------------------------------------ sp1hip_bb_poseidon2_permute

def test_permutation_of_edge_states(api):
    """The states of tests/test_bb31_arith.py through the kernel, against bb_py and against the C++ oracle."""
    states = edge_states()
    got = api.bb_poseidon2_permute(states)
    assert np.array_equal(got, permuted_edge_states())
    assert np.array_equal(got, orc.bb_permute(states))
    L, s = api._L(), api._stream_ptr()
    assert L.sp1hip_bb_poseidon2_permute(None, 0, s) == 0
    assert L.sp1hip_bb_poseidon2_permute(None, 1, s) != 0
