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


# ------------------------------------------------------------------------------------------------ edges (tests/test_outer_arith.py
# checks the field operations themselves; these check the kernels built from them)
_R1 = M.R256 % M.P                                           # Montgomery(1)


def _kat():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outer_poseidon2_kat.json")) as f:
        v = json.load(f)["vectors"]
    return [([int(x, 16) for x in t["input"]], [int(x, 16) for x in t["output"]]) for t in v]


def _edge_states():
    """Raw 24-word states: the host test's edge states, then every combination of lanes p - 1, 0, R mod p, p - (R mod p),
    taken both as canonical values (Montgomery-encoded) and as raw Montgomery words."""
    canon = [[0, 0, 0], [M.P - 1] * 3, [1, 0, 0], [0, 0, M.P - 1]] + [v for v, _ in _kat()] + [M.KNOWN_ANSWER_IN]
    lanes = [0, M.P - 1, _R1, M.P - _R1]
    words = [np.concatenate([M.to_words(x) for x in s]) for s in canon]
    for a in lanes:
        for b in lanes:
            for c in lanes:
                words.append(np.concatenate([M.to_words(x) for x in (a, b, c)]))
                words.append(np.array([(x >> (32 * i)) & 0xFFFFFFFF for x in (a, b, c) for i in range(8)]))
    return np.stack(words).astype(np.uint32)


def _host_permute_words(states):
    from sp1_amd import _lib
    out = np.ascontiguousarray(states, dtype=np.uint32).copy()
    assert _lib.load().sp1hip_outer_poseidon2_permute_host(out.ctypes.data_as(_lib.u32p), out.shape[0]) == 0
    return out


def _device_permute_words(api, states):
    d = api.to_device(np.ascontiguousarray(states, dtype=np.uint32))
    api.outer_poseidon2_permute(d)
    return api.to_host(d, states.shape)


def test_device_permutation_known_answers(api):
    """Both published vectors (HorizenLabs permute([0, 1, 2]) and the gnark test's permute([0, 0, 0])) on the device, in both
    limb-product forms, and on the host and in the model."""
    kats = _kat() + [(M.KNOWN_ANSWER_IN, M.KNOWN_ANSWER_OUT)]
    states = np.stack([np.concatenate([M.to_words(x) for x in i]) for i, _ in kats]).astype(np.uint32)
    for got in (_device_permute_words(api, states), _host_permute_words(states)):
        assert [[M.from_words(g[8 * k:8 * k + 8]) for k in range(3)] for g in got] == [o for _, o in kats]
    assert all(M.permute(i) == o for i, o in kats)


@pytest.mark.parametrize("form", ["mad", "lohi"])
def test_device_permutation_edge_states(api, monkeypatch, form):
    """Edge states through the device permutation in both forms (SP1HIP_OUTER_MUL is read on every call): word for word the
    host permutation's result, and the model's."""
    if form == "lohi":
        monkeypatch.setenv("SP1HIP_OUTER_MUL", "lohi")
    else:
        monkeypatch.delenv("SP1HIP_OUTER_MUL", raising=False)
    states = _edge_states()
    got = _device_permute_words(api, states)
    assert np.array_equal(got, _host_permute_words(states))
    for k in range(0, states.shape[0], 7):
        x = [M.from_words(states[k, 8 * j:8 * j + 8]) for j in range(3)]
        assert [M.from_words(got[k, 8 * j:8 * j + 8]) for j in range(3)] == M.permute(x), k


def test_device_permutation_lohi_equals_mad(api, monkeypatch):
    """The mul_lo / mul_hi form against the multiply-add form on 2^14 random and edge states: identical words."""
    rng = np.random.default_rng(21)
    raw = rng.integers(0, 1 << 32, (1 << 14, 24), dtype=np.uint64).astype(np.uint32)
    raw[:, 7::8] %= 0x30644E72
    states = np.concatenate([_edge_states(), raw])
    monkeypatch.delenv("SP1HIP_OUTER_MUL", raising=False)
    mad = _device_permute_words(api, states)
    monkeypatch.setenv("SP1HIP_OUTER_MUL", "lohi")
    lohi = _device_permute_words(api, states)
    assert np.array_equal(mad, lohi)
    assert np.array_equal(mad[:512], _host_permute_words(states[:512]))


# ------------------------------------------------------------------------------------------------ whole trees across the tail
_KB_R_INV = pow(1 << 32, -1, KB_P)


def _canon_rows(tables):
    """Row-major canonical KoalaBear values of the concatenated tables (Montgomery words in)."""
    w = np.concatenate(tables, axis=1).astype(np.uint64)
    return (w % KB_P) * _KB_R_INV % KB_P


def _bn_words(vals):
    """Canonical BN254 ints -> [n][8] Montgomery words."""
    blob = b"".join((v * M.R256 % M.P).to_bytes(32, "little") for v in vals)
    return np.frombuffer(blob, dtype="<u4").reshape(-1, 8)


def _host_tree(tables):
    """The whole tree as device words (leaf layer first) plus (root, commitment) as canonical ints: outer_model's structure
    (hash_row blocks of 16 columns, chunk j of 8 overwriting lane j, pairing, commitment), with the permutations done in
    batches by the host permutation of the library (an independent __int128 formulation, pinned to the model)."""
    canon = _canon_rows(tables)
    h, width = canon.shape
    st = np.zeros((h, 24), np.uint32)
    for b in range(0, width, 16):
        for j, c0 in enumerate(range(b, min(b + 16, width), 8)):
            chunk = canon[:, c0:min(c0 + 8, b + 16, width)].tolist()
            st[:, 8 * j:8 * j + 8] = _bn_words([M.reduce_31(r) for r in chunk])
        st = _host_permute_words(st)
    layers = [st[:, :8]]
    while layers[-1].shape[0] > 1:
        cur = layers[-1]
        x = np.zeros((cur.shape[0] // 2, 24), np.uint32)
        x[:, :8], x[:, 8:16] = cur[0::2], cur[1::2]
        layers.append(_host_permute_words(x)[:, :8])
    root = M.from_words(layers[-1][0])
    return np.concatenate(layers), root, M.commitment(root, h.bit_length() - 1, width)


def _edge_rows(t, seed):
    """Rows of a commitment at the edges: all zero, all canonical p_KB - 1, all Montgomery one, all raw word p_KB - 1."""
    t = t.copy()
    h = t.shape[0]
    rows = [0, h - 1, h // 2, (seed * 37) % h]
    for r, v in zip(rows, [0, M.kb_to_monty(KB_P - 1), M.kb_to_monty(1), KB_P - 1]):
        t[r] = v
    return t


def _commit_whole(api, tables):
    d = [api.ColMajor.from_row_major_host(t) for t in tables]
    commit, data = api.OuterMerkleTcsProver().commit_tensors(d)
    tree, root, com = _host_tree(tables)
    assert np.array_equal(api.to_host(data.tree, (-1, 8)), tree)
    assert M.from_words(data.root) == root and M.from_words(commit) == com
    return d, data, tree


@pytest.mark.parametrize("lg,widths", [(10, [5, 20]), (11, [8, 1, 9, 13]), (12, [24]), (10, [1, 2, 3] * 13 + [2])])
def test_whole_tree_across_the_tail_switch(api, lg, widths):
    """Every node, the root and the commitment at 2^10 (one layer launch, then a tail of 512), 2^11 (two) and 2^12 (three),
    with edge rows in every table."""
    rng = np.random.default_rng(100 + lg + len(widths))
    _commit_whole(api, [_edge_rows(_kb_table(rng, 1 << lg, w), k) for k, w in enumerate(widths)])


def test_whole_tree_against_the_model_at_2_10(api):
    """The same comparison with the pure model at 2^10 x 9 (two chunks in one block)."""
    rng = np.random.default_rng(110)
    tables = [_edge_rows(_kb_table(rng, 1 << 10, 9), 0)]
    _, _, tree = _commit_whole(api, tables)
    layers, _, _ = M.merkle_tree(tables)
    assert np.array_equal(tree, M.tree_words(layers))


@pytest.mark.parametrize("widths", [[16], [24], [32], [1000], [1, 2, 3] * 13 + [1], [3, 1, 2] * 13 + [3]])
def test_commit_wide_and_many_narrow_tensors(api, widths):
    """Widths 16, 24, 32 (exact blocks, a short last block of 8) and 1000 (62 blocks + 8), and 40 tensors of widths 1 to 3
    whose chunks straddle tensors many times over; edge rows in every table; checked against the pure model."""
    rng = np.random.default_rng(sum(widths) + len(widths))
    _commit_and_check(api, [_edge_rows(_kb_table(rng, 16, w), k) for k, w in enumerate(widths)])


def test_openings_at_every_index_of_a_2_10_tree(api):
    rng = np.random.default_rng(13)
    lg = 10
    tables = [_edge_rows(_kb_table(rng, 1 << lg, 5), 1), _edge_rows(_kb_table(rng, 1 << lg, 6), 2)]
    d, data, tree = _commit_whole(api, tables)
    prover = api.OuterMerkleTcsProver()
    idx = list(range(1 << lg))
    vals = prover.compute_openings_at_indices(d, idx)
    assert np.array_equal(vals, np.concatenate(tables, axis=1))
    proof = prover.prove_openings_at_indices(data, idx)
    offs = [sum(1 << (lg - j) for j in range(k)) for k in range(lg)]
    for i in idx:
        assert np.array_equal(proof["paths"][i], tree[[offs[k] + ((i >> k) ^ 1) for k in range(lg)]]), i
    paths = [[M.from_words(p) for p in q] for q in proof["paths"]]
    root, com = M.from_words(data.root), M.from_words(data.commit)
    assert M.verify_tensor_openings(com, root, lg, 11, idx, vals, paths)
    q = 613
    bad = [list(p) for p in paths[q:q + 1]]
    bad[0][7] = (bad[0][7] + 1) % M.P
    assert not M.verify_tensor_openings(com, root, lg, 11, [q], vals[q:q + 1], bad)
    bad_vals = vals[q:q + 1].copy()
    bad_vals[0, 4] = (int(bad_vals[0, 4]) + 1) % KB_P
    assert not M.verify_tensor_openings(com, root, lg, 11, [q], bad_vals, paths[q:q + 1])


@pytest.mark.parametrize("lb", [1, 3])
@pytest.mark.parametrize("lg_n", [0, 1, 5])
def test_outer_commit_mles_shapes(api, lg_n, lb):
    """commit_mles at lb 1 and 3, lg_n 0, 1 and 5, mixed widths: the inner codewords, committed as commit_tensors commits
    them, and (at the small shapes) the model's root and commitment."""
    rng = np.random.default_rng(10 * lg_n + lb)
    widths = [1, 9, 7, 16]
    mles = [api.ColMajor.from_row_major_host(_edge_rows(_kb_table(rng, 1 << lg_n, w), k)) for k, w in enumerate(widths)]
    commit, cws, data = api.outer_commit_mles(mles, lb)
    _, pd = api.BasefoldProver(lb, 16, 8).commit_mles(mles)
    for k in range(len(mles)):
        assert torch.equal(cws[k].words, pd.codeword(k).words), k
    commit2, data2 = api.OuterMerkleTcsProver().commit_tensors(cws)
    assert np.array_equal(commit, commit2)
    assert torch.equal(data.tree, data2.tree)
    host = [c.to_row_major_host() for c in cws]
    tree, root, com = _host_tree(host)
    assert np.array_equal(api.to_host(data.tree, (-1, 8)), tree)
    assert M.from_words(commit) == com
    if lg_n + lb <= 4:
        _, mroot, mcom = M.merkle_tree(host)
        assert (mroot, mcom) == (root, com)
