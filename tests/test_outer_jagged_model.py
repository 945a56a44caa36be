"""CPU checks of tests/outer_jagged_model.py, the hash-generic jagged PCS model the outer GPU prover is compared with, and of
the jagged part of the reference's real wrap proof (tests/golden/outer_wrap_jagged.npz + outer_wrap_basefold.npz):
  1. the two jagged wraps of the real proof reproduce: compress(stacked commitment, hash([n, rows.., cols..])) under the outer
     sponge is the vk's preprocessed_commit (round 0) and the proof's main_commitment (round 1);
  2. the model's INNER instance gives pyoracle.jagged_commit_wrap / jagged_prove bytes byte for byte on small shapes (one and
     two rounds, a zero-row table in the middle, a single-column round), so the model's protocol logic is pinned without any
     outer code;
  3. the model's OUTER verifier accepts the real JaggedPcsProof from the challenger state recorded at jagged entry (column
     claims, both sumchecks, the branching program, expected_eval, the batch evaluations, BaseFold on the first 12 queries) and
     names the failing check for one flip each in a row count, a column claim, a jagged sumcheck coefficient, a jagged-eval
     coefficient, expected_eval and a batch evaluation;
  4. the new entry points are declared in include/sp1hip.h and sp1_amd/_lib.py with the same number of arguments."""
import copy
import os
import re

import numpy as np
import pytest

import outer_basefold_model as BM
import outer_jagged_model as JM
import outer_model as M
import pyoracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LOG_BLOWUP, POW_BITS, NQ_KEEP = 3, 22, 12


def _fixtures():
    return np.load(os.path.join(HERE, "golden", "outer_wrap_jagged.npz")), np.load(os.path.join(HERE, "golden", "outer_wrap_basefold.npz"))


def _int(b):
    return int.from_bytes(bytes(bytearray(b)), "little")


def test_the_real_proofs_jagged_wraps_reproduce():
    j, b = _fixtures()
    for r, want in ((0, b["vk_preprocessed_commit"]), (1, b["main_commitment"])):
        counts = j["counts%d" % r]
        rows, cols = [int(x) for x in counts[:, 0]], [int(x) for x in counts[:, 1]]
        assert JM.jagged_wrap(BM.OUTER, _int(b["commits"][r]), rows, cols) == _int(want)
        # ... and the last two tables are the padding tables the counts of the real ones imply
        erows, ecols, padded, _ = JM.jagged_counts(list(zip(rows[:-2], cols[:-2])), int(j["max_log_row_count"]), 21)
        assert (erows, ecols) == (rows, cols) and padded == j["batch%d" % r].shape[0] << 21


@pytest.mark.parametrize("rounds,L,lsh,batch", [
    ([[(8, 3), (5, 2)]], 3, 2, 2),                                  # one round
    ([[(4, 1)], [(8, 2), (3, 1)]], 3, 2, 3),                        # two rounds, the first a single column
    ([[(8, 3), (0, 2), (5, 2)]], 3, 2, 2),                          # a zero-row table in the middle
    ([[(16, 2), (0, 5), (7, 3)], [(1, 1), (16, 1)]], 4, 3, 2),      # L > lsh, a table of one row
])
def test_inner_instance_equals_the_oracle_byte_for_byte(rounds, L, lsh, batch):
    lb, nq, pow_bits = 1, 3, 2
    z_row = orc.random_felts((L, 4), seed=99)
    o_ch, m_ch = orc.Challenger(), BM.INNER.challenger()
    o_rounds, m_rounds, o_claims, m_claims = [], [], [], []
    for ri, shapes in enumerate(rounds):
        tabs = [orc.random_felts((r, c), seed=10 * ri + i) if r else np.zeros((0, c), np.uint32) for i, (r, c) in enumerate(shapes)]
        o = orc.JaggedRound(tabs, L, lsh, batch, lb)
        m = JM.JaggedRound(BM.INNER, [orc.from_monty(t) for t in tabs], L, lsh, batch, lb)
        assert [int(x) for x in orc.from_monty(o.commit)] == m.commit
        wrap = orc.jagged_commit_wrap(orc.to_monty(np.array(m.stacked_commit, np.uint32)), [r for r, _ in shapes],
                                      [c for _, c in shapes], m.num_added_vals, L)
        assert [int(x) for x in orc.from_monty(wrap)] == m.commit
        cl = np.concatenate([orc.padded_column_openings(t, L, z_row) for t in tabs])
        o_rounds.append(o)
        m_rounds.append(m)
        o_claims.append(cl)
        m_claims.append(orc.from_monty(cl).tolist())
        o_ch.observe(o.commit)
        for x in m.commit:
            m_ch.observe(x)
    v_ch = m_ch.clone()
    want = orc.jagged_prove(z_row, o_claims, o_rounds, lsh, o_ch, lb, nq, pow_bits)
    z = orc.from_monty(z_row).tolist()
    got = JM.jagged_prove(BM.INNER, z, m_claims, m_rounds, m_ch, lb, nq, pow_bits)
    assert got == want
    assert [int(x) for x in orc.from_monty(o_ch.sample_ext())] == BM._sample_ext(m_ch)
    assert JM.jagged_verify(BM.INNER, [m.commit for m in m_rounds], z, m_claims, got, lsh, v_ch, lb, nq, pow_bits) == "ok"


def _real():
    j, b = _fixtures()
    sc = {}
    for tag in ("js", "je"):
        sc[tag] = dict(polys=j[tag + "_polys"].astype(np.int64).tolist(), claimed_sum=[int(x) for x in j[tag + "_claimed_sum"]],
                       point=j[tag + "_point"].astype(np.int64).tolist(), eval=[int(x) for x in j[tag + "_eval"]])
    p = dict(batch_evaluations=[j["batch0"].astype(np.int64).tolist(), j["batch1"].astype(np.int64).tolist()], sumcheck=sc["js"],
             jagged_eval=sc["je"], counts=[[(int(a), int(c)) for a, c in j["counts%d" % r]] for r in range(2)],
             merkle_tree_commitments=[_int(b["commits"][0]), _int(b["commits"][1])],
             expected_eval=[int(x) for x in j["expected_eval"]], max_log_row_count=int(j["max_log_row_count"]), log_m=int(j["log_m"]),
             basefold=bytes(bytearray(b["basefold_proof_q12"])))
    ch = M.Challenger()
    ch.sponge = [_int(x) for x in j["entry_sponge"]]
    ch.inp, ch.out = [int(x) for x in j["entry_inp"]], [int(x) for x in j["entry_out"]]
    commitments = [_int(b["vk_preprocessed_commit"]), _int(b["main_commitment"])]
    claims = [j["claims0"].astype(np.int64).tolist(), j["claims1"].astype(np.int64).tolist()]
    return p, BM._OuterChallenger(ch), commitments, j["z_row"].astype(np.int64).tolist(), claims


def _verify(p, ch, commitments, z_row, claims):
    return JM.jagged_verify_fields(BM.OUTER, commitments, z_row, claims, p, 21, ch, LOG_BLOWUP, NQ_KEEP, POW_BITS)


def test_outer_verifier_accepts_the_real_jagged_proof():
    p, ch, commitments, z_row, claims = _real()
    assert p["log_m"] == 27 and len(p["sumcheck"]["polys"]) == 27 and len(p["jagged_eval"]["polys"]) == 56
    assert [len(c) for c in p["counts"]] == [11, 11] and [len(x) for x in p["batch_evaluations"]] == [16, 23]
    assert _verify(p, ch, commitments, z_row, claims) == "ok"


def _flip_row_count(p, claims):
    a, c = p["counts"][1][0]
    p["counts"][1][0] = (a ^ 1, c)


def _flip_claim(p, claims):
    claims[1][3][2] ^= 1


def _flip_js(p, claims):
    p["sumcheck"]["polys"][5][1][0] ^= 1


def _flip_je(p, claims):
    p["jagged_eval"]["polys"][40][2][3] ^= 1


def _flip_expected(p, claims):
    p["expected_eval"][1] ^= 1


def _flip_batch(p, claims):
    p["batch_evaluations"][1][7][0] ^= 1


@pytest.mark.parametrize("flip,names", [(_flip_row_count, ("Shape", "CommitmentWrap")), (_flip_claim, ("ColumnClaims",)),
                                        (_flip_js, ("JaggedSumcheckPoint", "JaggedSumcheckRound")),
                                        (_flip_je, ("JaggedEvalSumcheckPoint", "JaggedEvalSumcheckRound")),
                                        (_flip_expected, ("ExpectedEval",)), (_flip_batch, ("BatchEvaluations",))])
def test_outer_verifier_rejects_one_flip(flip, names):
    p, ch, commitments, z_row, claims = _real()
    p, claims = copy.deepcopy(p), copy.deepcopy(claims)
    flip(p, claims)
    assert _verify(p, ch, commitments, z_row, claims) in names


NEW = ["sp1hip_outer_stacked_commit", "sp1hip_outer_jagged_commit", "sp1hip_outer_stacked_data_free", "sp1hip_outer_stacked_data_info",
       "sp1hip_outer_stacked_batch", "sp1hip_outer_jagged_proof_size", "sp1hip_outer_jagged_prove"]


def test_new_symbols_are_declared_with_matching_signatures():
    from sp1_amd import _lib
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    protos = {name: args for name, _, args in _lib.PROTOTYPES}
    inner = {"sp1hip_outer_stacked_commit": "sp1hip_stacked_commit", "sp1hip_outer_jagged_commit": "sp1hip_jagged_commit",
             "sp1hip_outer_jagged_prove": "sp1hip_jagged_prove", "sp1hip_outer_stacked_batch": "sp1hip_stacked_batch",
             "sp1hip_outer_stacked_data_free": "sp1hip_stacked_data_free"}
    for name in NEW:
        m = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert m, name + " is not declared in include/sp1hip.h"
        assert name in protos, name + " has no prototype in sp1_amd/_lib.py"
        assert len(protos[name]) == m.group(1).count(",") + 1, name
        if name in inner:                            # mirrors the inner call argument for argument
            assert [str(a) for a in protos[name]] == [str(a) for a in protos[inner[name]]], name
    from sp1_amd import api
    for cls in ("OuterStackedPcsProver", "OuterJaggedProver"):
        assert hasattr(getattr(api, cls), "commit_multilinears")
    assert hasattr(api.OuterJaggedProver, "prove_trusted_evaluations")
