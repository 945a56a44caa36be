"""LogUp-GKR on arbitrary tables of the real chips' interaction programs, the CPU side (tests/gkr_real.py): the generator is
deterministic, the case list covers the shapes it claims, the dense oracle equals the sparse one and its verifier accepts every
case that tests/test_gpu_gkr_real.py compares the device with, the verifier still rejects a pair that does not mirror, and the
oracle's circuit output equals a Python-integer model of the first layer and the fraction tree on three small cases."""
import numpy as np
import pytest

import gkr_real as GR
import kb_py
import pyoracle as orc


def _heights(chips):
    return [c[1].shape[0] for c in chips]


@pytest.mark.parametrize("kind", ["rand", "edge"])
def test_generator_is_deterministic(kind):
    spec = [("Byte", 5, True), ("MemoryConst", 3, True), ("Range", 0, False), ("Range", 0, False)]
    a = GR.real_gkr_chips(spec, GR.source_of(kind, 31))
    b = GR.real_gkr_chips(spec, GR.source_of(kind, 31))
    c = GR.real_gkr_chips(spec, GR.source_of(kind, 32))
    assert [x[0].name for x in a] == ["Byte", "Byte~", "MemoryConst", "MemoryConst~", "Range", "Range#2"]
    for (pa, ma, qa), (pb, mb, qb) in zip(a, b):
        assert np.array_equal(pa.to_array(), pb.to_array()) and np.array_equal(ma, mb)
        assert (qa is None) == (qb is None) and (qa is None or np.array_equal(qa, qb))
    assert any(not np.array_equal(x[1], y[1]) for x, y in zip(a, c))
    assert a[0][1] is a[1][1] and a[2][2] is a[3][2] and a[2][2] is not None          # a chip and its mirror share their tables
    assert a[1][0].sends == a[0][0].receives and a[1][0].receives == a[0][0].sends
    assert int(a[0][1].max()) < GR.P
    with pytest.raises(AssertionError):
        GR.real_gkr_chips([("Byte", 1, False)], GR.source_of(kind, 1))


def test_cases_reach_the_shapes_they_claim():
    stats = {}
    for name in GR.CASES:
        for spec_name, _, _ in GR.CASES[name][0]:
            stats.setdefault(spec_name, GR.shape_stats(GR.program(spec_name)))
    top = lambda key: max(s[key] for s in stats.values())
    assert top("values") == 106 and stats["KeccakPermute"]["values"] == 106
    assert stats["ShaCompress"]["values"] == 25 and stats["ShaCompress"]["value_terms"] == 16 and top("value_terms") == 16
    assert top("folded") == 9 and stats["Add"]["folded"] == 9
    assert top("mult_terms") == 7 and stats["LoadX0"]["mult_terms"] == 7
    assert stats["Mul"]["mult_terms"] == 5 and stats["DivRem"]["mult_terms"] == 4
    assert stats["BaseAlu"]["mult_terms"] == 4 and stats["ExtAlu"]["mult_terms"] == 4
    assert stats["DivRem"]["const_mults"] > 0
    assert stats["DivRem"]["value_terms"] == 8 and stats["LoadX0"]["value_terms"] == 7
    live = set().union(*(s["live"] for s in stats.values()))
    # live counts 1 .. 3 never flush at pending == 4; 4 and 8 flush and leave no tail; 5, 6, 7 and 9 leave tails of one, two,
    # three and one behind one or two flushes; 105 and 106 run 26 flushes
    assert live >= set(range(1, 17)) | {25, 105, 106}
    assert {105, 106} <= stats["KeccakPermute"]["live"] | stats["KeccakPermuteControl"]["live"]
    assert top("weights_not_one") == stats["Bls12381AddAssign"]["weights_not_one"] == 244
    # the hand-written chips, for comparison: what the older kernel-level tests reach
    import gkr_chips
    hand = [GR.shape_stats(c[0]) for c in gkr_chips.make_gkr_chips(4, 3, True, 2) + gkr_chips.make_gkr_wide_chips(4, 13, 3)]
    assert max(s["values"] for s in hand) == 13 and max(s["mult_terms"] for s in hand) == 1 and max(s["value_terms"] for s in hand) == 2
    assert sum(s["interactions"] for s in hand) == 7


def test_case_sizes():
    k = {name: GR.num_interactions(GR.case(name)[0]) for name in GR.CASES}
    assert k["core-rand"] == k["core-edge"] == 1138
    assert (k["k16"], k["k17"], k["k5"]) == (16, 17, 5)
    core = GR.case("core-rand")[0]
    assert [c[0].name for c in core] == sorted(c[0].name for c in core) and len(core) == 60
    assert [c[1].shape[0] for c in sorted(core, key=lambda c: c[0].name.rstrip("~")) if not c[0].name.endswith("~")] == \
        [GR.HEIGHTS[i % 17] for i in range(30)]
    assert GR.case("k17")[0][-2][1].shape[0] == 0 and GR.case("k17")[0][-2][0].name == "Range#2"
    assert max(c[0].main_width for c in GR.case("wide-edge")[0]) == 2640
    assert any(c[2] is not None and c[2].shape[0] for c in GR.case("recursion-edge")[0])


@pytest.mark.parametrize("name", list(GR.CASES))
def test_dense_oracle_equals_sparse_and_verifies(name):
    chips, L, want, state = GR.oracle_proof(name)
    ch = GR.seeded(orc.Challenger(), L)
    orc.set_gkr_sparse(True)
    try:
        sparse = orc.gkr_prove(chips, L, ch)
    finally:
        orc.set_gkr_sparse(False)
    assert sparse == want, GR.first_difference(sparse, want)
    assert np.array_equal(ch.state(), state)
    assert orc.gkr_verify(chips, _heights(chips), L, want, GR.seeded(orc.Challenger(), L)) == 0
    point, opened = _parse(want)
    assert point.shape == (L, 4) and [o[0] for o in opened] == [c[0].name for c in chips]


def _parse(blob):
    from sp1_amd import api
    return api.parse_logup_gkr_proof(blob)


@pytest.mark.parametrize("kind", ["rand", "edge"])
def test_verifier_rejects_a_pair_that_does_not_mirror(kind):
    """One cell of the mirror's table differs from the chip's, in a column that a value reads: the two fractions of that row no
    longer cancel and the verifier stops at the cumulative sum. Without this, the acceptance above would say nothing."""
    L = 4
    chips = GR.real_gkr_chips([("Byte", 5, True), ("Program", 9, True), ("Range", 3, True)], GR.source_of(kind, 41))
    ok = orc.gkr_prove(chips, L, GR.seeded(orc.Challenger(), L))
    assert orc.gkr_verify(chips, _heights(chips), L, ok, GR.seeded(orc.Challenger(), L)) == 0
    k = next(i for i, c in enumerate(chips) if c[0].name == "Program~")
    prog, main, prep = chips[k]
    _, values, mult = (prog.sends + prog.receives)[0]
    read = [(t[0], t[1]) for v in values for t in v.terms]
    assert read and mult.terms
    which, col = read[-1]
    main2, prep2 = main.copy(), prep.copy() if prep is not None else None
    table = main2 if which == "main" else prep2
    table[4, col] = (int(table[4, col]) + 1) % GR.P
    mcol = mult.terms[0]
    assert int((main if mcol[0] == "main" else prep)[4, mcol[1]]) != 0
    broken = chips[:k] + [(prog, main2, prep2)] + chips[k + 1:]
    blob = orc.gkr_prove(broken, L, GR.seeded(orc.Challenger(), L))
    assert orc.gkr_verify(broken, _heights(broken), L, blob, GR.seeded(orc.Challenger(), L)) != 0


MODEL_CASES = {
    "lookups": ([("Byte", 5, True), ("Program", 3, True), ("Range", 1, True), ("MemoryLocal", 6, True)], 3),
    "sha-loadx0": ([("ShaCompressControl", 7, True), ("LoadX0", 2, True)], 3),
    "keccak": ([("KeccakPermute", 3, True)], 2),           # betas up to index 106
}


@pytest.mark.parametrize("kind", ["rand", "edge"])
@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_circuit_output_equals_the_integer_model(name, kind):
    spec, L = MODEL_CASES[name]
    chips = GR.real_gkr_chips(spec, GR.source_of(kind, 51 + L))
    assert sum(c[0].num_interactions * c[1].shape[0] for c in chips) < 1000
    blob = orc.gkr_prove(chips, L, GR.seeded(orc.Challenger(), L))
    proof = GR.decode_proof(blob)
    ch = kb_py.Challenger()
    ch.observe_many(orc.from_monty(orc.random_felts((9,), L)).tolist())
    numerator, denominator = GR.circuit_output_model(chips, L, ch, proof["witness"])
    assert len(numerator) == len(proof["numerator"]) == 2 << (GR.num_interactions(chips) - 1).bit_length()
    assert numerator == proof["numerator"].tolist()
    assert denominator == proof["denominator"].tolist()
    if name == "keccak":
        assert GR.shape_stats(chips[0][0])["values"] == 106
