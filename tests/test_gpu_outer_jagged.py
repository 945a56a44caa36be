"""GPU parity (-m gpu) of the outer (BN254) stacked + jagged PCS: sp1hip_outer_stacked_commit, sp1hip_outer_jagged_commit and
sp1hip_outer_jagged_prove against the OUTER instance of tests/outer_jagged_model.py — commitments, counts, proof bytes and the
final challenger state equal, and the model verifier accepts every proof. The model is pinned by
tests/test_outer_jagged_model.py (the oracle's bytes for its inner instance, the reference's real wrap proof for its outer
verifier).

Sizes of the model-compared cases: log_stacking_height <= 4, log_blowup <= 3, at most 9 stacked columns per round, 4 queries,
3 proof-of-work bits, so a round's tree has at most 2^7 leaves. The Python model side (commit + prove + verify) of the largest
of them takes about 0.8 s on one CPU core and all of them together about 2.5 s (measured without a GPU).

The wrap-shape case (the real proof's (rows, cols) of both rounds, 2^24-leaf trees, wrap_fri_config: blowup 8, 94 queries, 22
bits) is checked by the model VERIFIER only, which needs the openings and not the trees: about 30,000 Python permutations. Its
Merkle check is the large-index comparison the feature asks for: hash_row of the 16 / 23 opened words of each of the 94
sampled leaves of a 2^24-row codeword, walked up the 24 opened siblings, must give the root, and compress(root, hash([24,
width])) the commitment — the host-side permutation at sampled leaves and up their paths against the device's leaf layer,
layers and tail."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import os  # noqa: E402

import outer_basefold_model as BM  # noqa: E402
import outer_jagged_model as JM  # noqa: E402
import outer_model as M  # noqa: E402
import pyoracle as orc  # noqa: E402

P = BM.P
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _tables(shapes, seed, fill=None):
    out = []
    for k, (h, w) in enumerate(shapes):
        if not h:
            out.append(np.zeros((0, w), np.uint32))
        elif fill is None:
            out.append(orc.random_felts((h, w), seed + k))
        else:
            out.append(orc.to_monty(np.full((h, w), fill, np.uint32)))
    return out


def _dev(api, tabs):
    return [api.ColMajor.from_row_major_host(t) if t.shape[0] else api.ColMajor(torch.zeros(0, dtype=torch.int32, device="cuda"), 0, t.shape[1])
            for t in tabs]


def _canon(tabs):
    return [orc.from_monty(t) if t.shape[0] else t for t in tabs]


COMMIT_CASES = [
    ([(0, 3), (8, 2), (5, 3)], 3, 2, 2),             # a zero-row table first
    ([(8, 2), (0, 3), (5, 3)], 3, 2, 2),             # ... in the middle
    ([(8, 2), (5, 3), (0, 4)], 3, 2, 3),             # ... last
    ([(1, 1), (7, 2)], 3, 3, 2),                     # a table of one row
    ([(8, 2), (4, 4)], 3, 3, 2),                     # area 32 = 4 x 2^3: nothing added, the padding table's minimum one column
    ([(3, 1), (2, 1)], 2, 4, 2),                     # 11 values added, 4-row padding tables: several padding columns
]


@pytest.mark.parametrize("shapes,L,lsh,batch", COMMIT_CASES)
def test_outer_stacked_and_jagged_commit_match_the_model(api, shapes, L, lsh, batch):
    lb = 1
    tabs = _tables(shapes, 5)
    m = JM.JaggedRound(BM.OUTER, _canon(tabs), L, lsh, batch, lb)
    commit, sd, added = api.OuterStackedPcsProver(lsh, batch, lb).commit_multilinears(_dev(api, [t for t in tabs if t.shape[0]]))
    assert M.from_words(commit) == m.stacked_commit and added == m.num_added_vals
    assert sd.padded_area == m.padded and [b.width for b in sd.batches] == [len(x[0]) for x in m.pcs.mles]
    jcommit, jd = api.OuterJaggedProver(L, lsh, batch, lb).commit_multilinears(_dev(api, tabs))
    assert M.from_words(jd.commit) == m.stacked_commit
    assert M.from_words(jcommit) == m.commit and np.array_equal(jcommit, jd.jagged_commit)
    assert jd.row_counts == m.rows and jd.column_counts == m.cols


PROVE_CASES = [
    # rounds of (rows, cols), max_log_row_count, log_stacking_height, batch, log_blowup, fill, zero coordinate of z_row
    ([[(8, 3), (5, 2)]], 3, 2, 2, 1, None, None),                                    # one round, L above lsh
    ([[(16, 2), (0, 3), (7, 1)], [(16, 4), (1, 2), (9, 3)]], 4, 3, 2, 1, None, None),    # preprocessed + main
    ([[(6, 2), (6, 2), (0, 1), (0, 4)]], 3, 4, 3, 1, None, None),                    # L below lsh
    ([[(8, 1)], [(8, 3), (3, 2)]], 3, 3, 2, 3, None, None),                          # L equal to lsh, blowup 8
    ([[(8, 3), (5, 2)]], 3, 2, 2, 1, 0, None),                                       # all-zero tables
    ([[(8, 2)], [(7, 2), (4, 1)]], 3, 2, 2, 3, P - 1, None),                         # all-(p - 1) tables, blowup 8
    ([[(8, 3), (5, 2)]], 3, 2, 2, 1, None, 1),                                       # z_row with a zero coordinate
]


def _setup(api, rounds, L, lsh, batch, lb, fill, seed=11):
    jp = api.OuterJaggedProver(L, lsh, batch, lb)
    g_ch, m_ch = api.OuterChallenger(), BM.OUTER.challenger()
    g_rounds, m_rounds, tabs_all = [], [], []
    for r, shapes in enumerate(rounds):
        tabs = _tables(shapes, seed + 100 * r, fill)
        m = JM.JaggedRound(BM.OUTER, _canon(tabs), L, lsh, batch, lb)
        c, sd = jp.commit_multilinears(_dev(api, tabs))
        assert M.from_words(c) == m.commit
        g_ch.observe_commitment(c)
        m_ch.observe_digest(m.commit)
        g_rounds.append(sd)
        m_rounds.append(m)
        tabs_all.append(tabs)
    return jp, g_ch, m_ch, g_rounds, m_rounds, tabs_all


@pytest.mark.parametrize("rounds,L,lsh,batch,lb,fill,zero_at", PROVE_CASES)
def test_outer_jagged_proof_matches_the_model(api, rounds, L, lsh, batch, lb, fill, zero_at):
    nq, pw = 4, 3
    jp, g_ch, m_ch, g_rounds, m_rounds, tabs_all = _setup(api, rounds, L, lsh, batch, lb, fill)
    z_row = g_ch.sample_point(L)
    assert orc.from_monty(z_row).tolist() == [BM._sample_ext(m_ch) for _ in range(L)]
    if zero_at is not None:
        z_row[zero_at] = 0
    claims = [np.concatenate([orc.padded_column_openings(t, L, z_row) for t in tabs]) for tabs in tabs_all]
    z, m_claims = orc.from_monty(z_row).tolist(), [orc.from_monty(c).tolist() for c in claims]
    v_ch = m_ch.clone()
    want = JM.jagged_prove(BM.OUTER, z, m_claims, m_rounds, m_ch, lb, nq, pw)
    assert jp.proof_size(g_rounds, nq, pw) == len(want)
    got = jp.prove_trusted_evaluations(z_row, claims, g_rounds, g_ch, nq, pw)
    assert len(got) == len(want)
    assert got == want
    assert np.array_equal(g_ch.state(), m_ch.ch.state()), "final transcript state differs from the model's"
    assert JM.jagged_verify(BM.OUTER, [m.commit for m in m_rounds], z, m_claims, got, lsh, v_ch, lb, nq, pw) == "ok"


def test_outer_jagged_prove_size_protocol_and_failed_calls_keep_the_transcript(api):
    import ctypes as C
    rounds, L, lsh, batch, lb = [[(8, 3), (5, 2)]], 3, 2, 2, 1
    nq, pw = 4, 3
    jp, g_ch, _, g_rounds, _, tabs_all = _setup(api, rounds, L, lsh, batch, lb, None)
    z_row = orc.random_felts((L, 4), 1)
    claims = [np.concatenate([orc.padded_column_openings(t, L, z_row) for t in tabs]) for tabs in tabs_all]
    before = g_ch.state()
    size = jp.proof_size(g_rounds, nq, pw)
    lib = api._L()
    args = jp._args(z_row, claims, g_rounds, g_ch, nq, pw)
    for cap, buf in ((0, None), (size - 1, (C.c_uint8 * size)())):
        n = C.c_size_t(cap)
        assert lib.sp1hip_outer_jagged_prove(*args, buf, C.byref(n), None) == api._lib.ERROR_BUFFER_TOO_SMALL
        assert n.value == size
        assert np.array_equal(g_ch.state(), before), "a too-small buffer must leave the challenger untouched"
    with pytest.raises(api._lib.Sp1HipError):
        jp.prove_trusted_evaluations(z_row, [np.zeros((1, 4), np.uint32)], g_rounds, g_ch, nq, pw)      # wrong number of claims
    assert np.array_equal(g_ch.state(), before)
    other = api.OuterJaggedProver(L + 1, lsh, batch, lb)
    _, sd2 = other.commit_multilinears(_dev(api, tabs_all[0]))
    with pytest.raises(api._lib.Sp1HipError):                                                            # rounds disagree on parameters
        jp.prove_trusted_evaluations(z_row, claims + claims, g_rounds + [sd2], g_ch, nq, pw)
    assert np.array_equal(g_ch.state(), before)
    with pytest.raises(api._lib.Sp1HipError):                                                            # fails in the BaseFold opening
        jp.prove_trusted_evaluations(z_row, claims, g_rounds, g_ch, 0, pw)
    assert np.array_equal(g_ch.state(), before), "a failed call must leave the challenger untouched"
    with pytest.raises(api._lib.Sp1HipError):                                                            # no table value at all
        jp.commit_multilinears(_dev(api, _tables([(0, 3)], 1)))
    jp.prove_trusted_evaluations(z_row, claims, g_rounds, g_ch, nq, pw)
    assert not np.array_equal(g_ch.state(), before)


def test_inner_jagged_prove_still_gives_the_oracle_bytes(api):
    """The refactor guard: sp1hip_jagged_prove is now the inner instantiation of the shared round loop."""
    from test_oracle_jagged import CASES, claims_for, make_rounds
    for shapes, L, lsh, batch in (CASES[1], CASES[2]):
        lb, nq, pw = 1, 6, 4
        rounds, tabs = make_rounds(shapes, L, lsh, batch, 7 + L, lb)
        jp = api.JaggedProver(L, lsh, batch, lb)
        o_ch, g_ch, g_rounds = orc.Challenger(), api.DuplexChallenger(), []
        for r, tb in zip(rounds, tabs):
            c, sd = jp.commit_multilinears(_dev(api, tb))
            assert np.array_equal(r.commit, c)
            g_rounds.append(sd)
            o_ch.observe(c)
            g_ch.observe(c)
        z_row = o_ch.sample_point(L)
        g_ch.sample_point(L)
        claims = claims_for(tabs, L, z_row)
        want = orc.jagged_prove(z_row, claims, rounds, lsh, o_ch, lb, nq, pw)
        assert jp.prove_trusted_evaluations(z_row, claims, g_rounds, g_ch, nq, pw) == want
        assert np.array_equal(g_ch.state(), o_ch.state())


def test_outer_jagged_at_the_wrap_shape(api):
    """The real wrap proof's shape: 2 rounds x 11 tables, max_log_row_count = log_stacking_height = 21, blowup 8 (2^24-leaf
    trees of 16 and 23 columns), 94 queries, 22 proof-of-work bits; seeded random tables."""
    j = np.load(os.path.join(HERE, "golden", "outer_wrap_jagged.npz"))
    L, lsh, lb, nq, pw, batch = int(j["max_log_row_count"]), 21, 3, 94, 22, 64
    gen = torch.Generator(device="cuda").manual_seed(2024)
    jp = api.OuterJaggedProver(L, lsh, batch, lb)
    g_ch, m_ch = api.OuterChallenger(), BM.OUTER.challenger()
    g_rounds, commits, tabs_all = [], [], []
    for r in range(2):
        counts = [(int(a), int(c)) for a, c in j["counts%d" % r]]
        tabs = [api.ColMajor(torch.randint(0, P, (h * w,), dtype=torch.int32, device="cuda", generator=gen), h, w) for h, w in counts[:-2]]
        c, sd = jp.commit_multilinears(tabs)
        assert (sd.row_counts, sd.column_counts) == ([a for a, _ in counts], [b for _, b in counts]), "the real proof's padding tables"
        assert M.from_words(c) == JM.jagged_wrap(BM.OUTER, M.from_words(sd.commit), sd.row_counts, sd.column_counts)
        assert sd.padded_area >> lsh == j["batch%d" % r].shape[0]
        g_ch.observe_commitment(c)
        m_ch.observe_digest(M.from_words(c))
        g_rounds.append(sd)
        commits.append(c)
        tabs_all.append(tabs)
    z_row = g_ch.sample_point(L)
    [BM._sample_ext(m_ch) for _ in range(L)]
    bf = api.BasefoldProver(lb, nq, pw)
    claims = []
    for tabs in tabs_all:
        cl = []
        for t in tabs:
            if t.height == 1 << L:
                full = t
            else:
                w = torch.zeros((t.width, 1 << L), dtype=torch.int32, device="cuda")
                w[:, :t.height] = t.words.view(t.width, t.height)
                full = api.ColMajor(w.view(-1), 1 << L, t.width)
            cl.append(np.asarray(bf.evaluate_mles([full], z_row)).reshape(-1, 4))
        claims.append(np.concatenate(cl))
    got = jp.prove_trusted_evaluations(z_row, claims, g_rounds, g_ch, nq, pw)
    assert len(got) == jp.proof_size(g_rounds, nq, pw)
    p = JM.parse_proof(BM.OUTER, got)
    assert p["merkle_tree_commitments"] == [M.from_words(sd.commit) for sd in g_rounds]
    assert p["log_m"] == int(j["log_m"]) and [len(b) for b in p["batch_evaluations"]] == [16, 23]
    bfp = BM.parse_proof(BM.OUTER, p["basefold"])
    assert [o["lg_h"] for o in bfp["comps"]] == [24, 24] and [o["width"] for o in bfp["comps"]] == [16, 23]
    z, m_claims = orc.from_monty(z_row).tolist(), [orc.from_monty(c).tolist() for c in claims]
    assert JM.jagged_verify_fields(BM.OUTER, [M.from_words(c) for c in commits], z, m_claims, p, lsh, m_ch, lb, nq, pw) == "ok"
    assert np.array_equal(g_ch.state(), m_ch.ch.state()), "the verifier's transcript ends where the prover's does"
