"""CPU checks of tests/outer_basefold_model.py, the hash-generic BaseFold model the outer GPU prover is compared with:
  * instantiated with the inner primitives its proof bytes equal the C++ oracle's byte for byte (the oracle is pinned on the
    reference's real inner proof), so the protocol logic (batching, round loop, query phase, bincode) is pinned
    independently of any outer code;
  * instantiated with the outer primitives its verifier accepts the REAL BasefoldProof of the reference's wrap proof (first 12
    queries, tests/golden/outer_wrap_basefold.npz) from the challenger state the replay recorded at BaseFold entry, and rejects
    it with one flipped byte in a univariate message, a path digest, an opened value and final_poly;
  * and, in addition, accepts its own prover's bytes and names the failing check on the same flips."""
import os

import numpy as np
import pytest

import outer_basefold_model as BM
import pyoracle as orc

P = BM.P


def _tables(rng, dim, widths):
    return [rng.integers(0, P, (1 << dim, w), dtype=np.uint64).astype(np.uint32) for w in widths]


def _point(rng, dim):
    return [[int(x) for x in rng.integers(0, P, 4)] for _ in range(dim)]


def _claims(rounds_tables, point):
    return [e for tabs in rounds_tables for t in tabs for e in BM.eval_mle_columns(t.tolist(), point)]


@pytest.mark.parametrize("dim,lb,round_widths", [(1, 1, [[1]]), (2, 2, [[3, 2], [4]]), (4, 1, [[16, 10, 14], [20, 78, 34], [10, 10]]),
                                                   (5, 3, [[2], [1, 1]])])
def test_inner_instance_equals_the_oracle_byte_for_byte(dim, lb, round_widths):
    rng = np.random.default_rng(100 * dim + lb)
    tabs = [_tables(rng, dim, ws) for ws in round_widths]
    point = _point(rng, dim)
    claims = _claims(tabs, point)
    nq, pow_bits = 5, 6
    # model
    m_rounds = [BM.CommittedRound(BM.INNER, [t.tolist() for t in ts], lb) for ts in tabs]
    m_ch = BM.INNER.challenger()
    for r in m_rounds:
        m_ch.observe_digest(r.commit)
    blob = BM.basefold_prove(BM.INNER, point, m_rounds, claims, m_ch, lb, nq, pow_bits)
    # oracle (Montgomery words)
    o_rounds = [orc.CommittedRound([orc.to_monty(t) for t in ts], lb) for ts in tabs]
    o_ch = orc.Challenger()
    for r, mr in zip(o_rounds, m_rounds):
        assert orc.from_monty(r.commit).tolist() == mr.commit
        o_ch.observe(r.commit)
    o_claims, k = [], 0
    for ts in tabs:
        per = []
        for t in ts:
            per.append(orc.to_monty(np.array(claims[k:k + t.shape[1]], np.uint32)))
            k += t.shape[1]
        o_claims.append(per)
    want = orc.basefold_prove(orc.to_monty(np.array(point, np.uint32)), o_rounds, o_claims, o_ch, lb, nq, pow_bits)
    assert blob == want
    assert orc.from_monty(o_ch.state()[:16]).tolist() == m_ch.ch.state
    # and the model's verifier accepts what both wrote
    v = BM.INNER.challenger()
    for r in m_rounds:
        v.observe_digest(r.commit)
    per_round, k = [], 0
    for r in m_rounds:
        per_round.append(claims[k:k + r.width])
        k += r.width
    assert BM.basefold_verify(BM.INNER, [r.commit for r in m_rounds], point, per_round, blob, v, lb, nq, pow_bits) == "ok"


def _outer_instance():
    rng = np.random.default_rng(7)
    dim, lb, nq, pow_bits = 3, 1, 4, 4
    tabs = [_tables(rng, dim, [3]), _tables(rng, dim, [2, 2])]
    point = _point(rng, dim)
    claims = _claims(tabs, point)
    rounds = [BM.CommittedRound(BM.OUTER, [t.tolist() for t in ts], lb) for ts in tabs]
    ch = BM.OUTER.challenger()
    for r in rounds:
        ch.observe_digest(r.commit)
    start = ch.clone()
    blob = BM.basefold_prove(BM.OUTER, point, rounds, claims, ch, lb, nq, pow_bits)
    return dict(dim=dim, lb=lb, nq=nq, pow_bits=pow_bits, point=point, rounds=rounds, per_round=[claims[:3], claims[3:]],
                start=start, end=ch, blob=blob)


def test_outer_instance_verifies_and_flips_are_rejected():
    c = _outer_instance()

    def verify(blob):
        ch = c["start"].clone()
        res = BM.basefold_verify(BM.OUTER, [r.commit for r in c["rounds"]], c["point"], c["per_round"], blob, ch, c["lb"],
                                 c["nq"], c["pow_bits"])
        return res, ch

    res, ch = verify(c["blob"])
    assert res == "ok"
    assert np.array_equal(ch.ch.state(), c["end"].ch.state())
    blob, dim, nq = c["blob"], c["dim"], c["nq"]
    assert len(blob) == _outer_size(dim, [3, 4], c["lb"], nq)

    def flipped(off):
        b = bytearray(blob)
        b[off] ^= 1
        return bytes(b)

    uni_off = 8                                              # first word of the first univariate message
    assert verify(flipped(uni_off))[0].split(":")[0] in ("Sumcheck", "Pow", "Parse")
    comp0 = 8 + 32 * dim + 8 + 40 * dim + 8                  # first component opening: u64 count, then the values
    assert verify(flipped(comp0 + 8))[0].split(":")[0] in ("Tcs", "QueryValueMismatch", "Parse")
    path0 = comp0 + 8 + 4 * nq * 3 + 24 + 40 + 24            # first path digest of that opening (after its length prefix)
    assert verify(flipped(path0 + 8))[0].split(":")[0] in ("Tcs", "Parse")
    assert verify(flipped(len(blob) - 24))[0].split(":")[0] in ("Pow", "QueryFinalPolyMismatch", "SumcheckFinalPolyMismatch", "Parse")
    assert verify(flipped(path0))[0].startswith("Parse")     # the digest's length prefix


def _outer_size(dim, widths, lb, nq):
    def opening(w, lg_h):
        return 8 + 4 * nq * w + 24 + 40 + 24 + 40 * nq * lg_h + 24
    return (8 + 32 * dim + 8 + 40 * dim + 8 + sum(opening(w, dim + lb) for w in widths) + 8 +
            sum(opening(8, dim + lb - 1 - r) for r in range(dim)) + 16 + 8)


def test_outer_verifier_accepts_the_real_wrap_basefold_proof_and_rejects_flips():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outer_wrap_basefold.npz"))
    blob = g["basefold_proof_q12"].tobytes()
    commits = [int.from_bytes(bytes(c), "little") for c in g["commits"]]
    point = g["point"].tolist()
    claims = [g["claims0"].tolist(), g["claims1"].tolist()]
    dim, nq, lb, pow_bits = len(point), 12, 3, 22

    def start():
        ch = BM.OUTER.challenger()
        ch.ch.sponge = [int.from_bytes(bytes(x), "little") for x in g["entry_sponge"]]
        ch.ch.inp, ch.ch.out = g["entry_inp"].tolist(), g["entry_out"].tolist()
        return ch

    def verify(b):
        return BM.basefold_verify(BM.OUTER, commits, point, claims, b, start(), lb, nq, pow_bits)

    assert verify(blob) == "ok"

    def flipped(off, bit=1):
        b = bytearray(blob)
        b[off] ^= bit
        return bytes(b)

    # (a flip may also leave a word or digest non-canonical, which the parser rejects: admitted everywhere)
    assert verify(flipped(8)).split(":")[0] in ("Sumcheck", "Pow", "Parse")                     # a univariate message
    comp0 = 8 + 32 * dim + 8 + 40 * dim + 8
    assert verify(flipped(comp0 + 8)).split(":")[0] in ("Tcs", "QueryValueMismatch", "Parse")     # an opened value
    path0 = comp0 + 8 + 4 * nq * 16 + 24 + 40 + 24
    assert verify(flipped(path0 + 8)).split(":")[0] in ("Tcs", "Parse")                            # a path digest
    assert verify(flipped(len(blob) - 24)).split(":")[0] in ("Pow", "QueryFinalPolyMismatch", "SumcheckFinalPolyMismatch", "Parse")
