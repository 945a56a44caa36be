"""GPU checks (-m gpu) of the outer (BN254) commitment layer: the device Poseidon2-BN254 permutation against the host one, the
outer Merkle tensor commitment, openings and commit_mles against tests/outer_model.py (an independent restatement of the
specification in Python ints), and the device grind of the outer transcript against the host check_witness.
Model-compared sizes stay small: the model takes ~0.35 ms per permutation."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import outer_model as M  # noqa: E402

KB_P = M.KB_P


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _rand_bn(rng, n):
    return [int.from_bytes(rng.bytes(32), "little") % M.P for _ in range(n)]


def _kb_table(rng, h, w):
    return rng.integers(0, KB_P, (h, w), dtype=np.uint64).astype(np.uint32)       # Montgomery words are any value < p


def test_device_permutation_matches_host(api):
    from sp1_amd import _lib
    rng = np.random.default_rng(1)
    n = 1 << 16
    words = np.stack([np.concatenate([M.to_words(x) for x in _rand_bn(rng, 3)]) for _ in range(64)]).astype(np.uint32)
    states = np.resize(words, (n, 24))
    # most states: random Montgomery words drawn directly (any 8-word value < p)
    raw = rng.integers(0, 1 << 32, (n, 24), dtype=np.uint64).astype(np.uint32)
    raw[:, 7::8] %= 0x30644E72                                  # top word below p's: the value is < p
    states[64:] = raw[64:]
    states[0] = np.concatenate([M.to_words(x) for x in M.KNOWN_ANSWER_IN])
    d = api.to_device(states)
    api.outer_poseidon2_permute(d)
    got = api.to_host(d, (n, 24))
    want = states.copy()
    lib = _lib.load()
    assert lib.sp1hip_outer_poseidon2_permute_host(want.ctypes.data_as(_lib.u32p), n) == 0
    assert np.array_equal(got, want)
    assert [M.from_words(got[0, 8 * k:8 * k + 8]) for k in range(3)] == M.KNOWN_ANSWER_OUT
    assert [M.from_words(got[1, 8 * k:8 * k + 8]) for k in range(3)] == M.permute([M.from_words(states[1, 8 * k:8 * k + 8]) for k in range(3)])


def _commit_and_check(api, tables):
    d = [api.ColMajor.from_row_major_host(t) for t in tables]
    commit, data = api.OuterMerkleTcsProver().commit_tensors(d)
    layers, root, com = M.merkle_tree(tables)
    assert np.array_equal(api.to_host(data.tree, (-1, 8)), M.tree_words(layers))
    assert M.from_words(data.root) == root and M.from_words(commit) == com
    return d, data, layers


@pytest.mark.parametrize("width", [1, 7, 8, 9, 15, 16, 17, 100])
def test_commit_widths(api, width):
    rng = np.random.default_rng(width)
    _commit_and_check(api, [_kb_table(rng, 16, width)])


@pytest.mark.parametrize("widths", [[3, 6], [5, 5, 7], [1, 14, 2], [8, 1, 9]])
def test_commit_chunks_straddle_tensors(api, widths):
    rng = np.random.default_rng(sum(widths))
    _commit_and_check(api, [_kb_table(rng, 16, w) for w in widths])


@pytest.mark.parametrize("lg", [0, 1, 4, 9])
def test_commit_heights(api, lg):
    rng = np.random.default_rng(40 + lg)
    _commit_and_check(api, [_kb_table(rng, 1 << lg, 11), _kb_table(rng, 1 << lg, 6)])


def test_openings_verify_and_a_flipped_sibling_fails(api):
    rng = np.random.default_rng(9)
    tables = [_kb_table(rng, 64, 10), _kb_table(rng, 64, 13)]
    d, data, layers = _commit_and_check(api, tables)
    prover = api.OuterMerkleTcsProver()
    idx = [0, 63, 17, 40, 17]
    vals = prover.compute_openings_at_indices(d, idx)
    assert np.array_equal(vals, np.concatenate(tables, axis=1)[idx])
    proof = prover.prove_openings_at_indices(data, idx)
    paths = [[M.from_words(p) for p in q] for q in proof["paths"]]
    for q, i in enumerate(idx):
        assert paths[q] == [layers[k][(i >> k) ^ 1] for k in range(6)]
    root, com = M.from_words(data.root), M.from_words(data.commit)
    assert M.verify_tensor_openings(com, root, 6, 23, idx, vals, paths)
    bad = [list(p) for p in paths]
    bad[2][3] = (bad[2][3] + 1) % M.P
    assert not M.verify_tensor_openings(com, root, 6, 23, idx, vals, bad)


def test_large_commit_sampled_leaves_and_openings(api):
    """2^20 x 64: 256 sampled leaf digests equal the model, 64 openings verify against the returned root and commitment."""
    lg, w = 20, 64
    h = 1 << lg
    g = torch.Generator(device="cuda").manual_seed(3)
    words = torch.randint(0, KB_P, (w * h,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    t = api.ColMajor(words, h, w)
    prover = api.OuterMerkleTcsProver()
    commit, data = prover.commit_tensors([t])
    tree = data.tree.view(-1, 8)
    rng = np.random.default_rng(4)
    rows = np.concatenate([[0, h - 1], rng.integers(0, h, 254)]).astype(np.int64)
    cols = words.view(w, h)[:, torch.from_numpy(rows).cuda()].cpu().numpy().view(np.uint32).T
    leaves = api.to_host(tree[torch.from_numpy(rows).cuda()].reshape(-1)).reshape(-1, 8)
    for k in range(len(rows)):
        assert M.from_words(leaves[k]) == M.hash_row([M.kb_from_monty(v) for v in cols[k]]), k
    idx = [int(x) for x in rows[:64]]
    vals = prover.compute_openings_at_indices([t], idx)
    assert np.array_equal(vals, cols[:64])
    proof = prover.prove_openings_at_indices(data, idx)
    paths = [[M.from_words(p) for p in q] for q in proof["paths"]]
    assert M.verify_tensor_openings(M.from_words(commit), M.from_words(data.root), lg, w, idx, vals, paths)


def test_outer_commit_mles_reuses_the_inner_codewords(api):
    rng = np.random.default_rng(12)
    lg_n, lb, widths = 8, 2, [5, 12]
    mles = [api.ColMajor.from_row_major_host(_kb_table(rng, 1 << lg_n, w)) for w in widths]
    commit, cws, data = api.outer_commit_mles(mles, lb)
    _, pd = api.BasefoldProver(lb, 16, 8).commit_mles(mles)
    for k in range(len(mles)):
        assert torch.equal(cws[k].words, pd.codeword(k).words), k
    commit2, data2 = api.OuterMerkleTcsProver().commit_tensors(cws)
    assert np.array_equal(commit, commit2)
    assert torch.equal(data.tree, data2.tree)


# witness position in the sponge's input buffer for each bits value: covers both chunks, chunk boundaries and the 16th slot
_PREFIX = {1: 0, 2: 1, 3: 7, 4: 8, 5: 9, 6: 15, 7: 16, 8: 3, 9: 14, 10: 6, 11: 12, 12: 23, 13: 5, 14: 31, 15: 2, 16: 10}


@pytest.mark.parametrize("bits", list(range(1, 17)))
def test_device_grind(api, bits):
    ch = api.OuterChallenger()
    ch.observe([M.kb_to_monty((31 * i + bits) % KB_P) for i in range(_PREFIX[bits])])
    if bits % 3 == 0:
        ch.observe_commitment(M.to_words(12345 + bits))
        ch.sample()
    before = ch.clone()
    w = ch.grind(bits)
    ref = before.clone()
    assert ref.check_witness(bits, w)
    assert np.array_equal(ch.state(), ref.state())
    if bits <= 12:
        wc = M.kb_from_monty(w)
        for x in range(wc):
            assert not before.clone().check_witness(bits, M.kb_to_monty(x)), (bits, x)
