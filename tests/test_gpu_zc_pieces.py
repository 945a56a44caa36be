"""GPU parity (-m gpu) of the zerocheck's fused pieces on ARBITRARY tables of the real chips (tests/zc_arbitrary.py): `api.zerocheck`
against `orc.zerocheck_prove` on the same tables, proof bytes and final transcript state equal; no verifier leg, the tables satisfy
nothing. Every case is proved twice on the GPU — by the pieces and, under SP1HIP_ZC_MACRO=0, by the interpreter — so a mismatch
says which of oracle / interpreter / pieces stand apart. The whole-shard tests only ever show these kernels satisfying traces
(selectors 0 / 1, is_real = 0 padding, byte limbs, every constraint zero) at heights up to 704 rows.

Kernels and the numbers the heights are chosen against (plan_round and the launches of sp1_amd/csrc/zerocheck.hip):
  * default path: rounds 0 and 1 from one pass over row QUADS — zc_biv_macro_kernel<1 | 2 | 3 | 6>, zc_biv_keccak_kernel,
    zc_biv_poly_kernel, zc_biv_corner_kernel, min(ceil(quads / 256), 512) workgroups of 256 quads per piece (the corner kernel: per
    slice of ZC_CORNER_COLS = 32 columns; the widths 82, 241, 2,640, ... leave the last slice partial) — then from round 2 on row
    PAIRS of the folded tables: zc_macro_kernel<false, KIND> with min(ceil(pairs / 256), 512) workgroups, and for the identities
    zc_poly_kernel<false> (a lane per pair) while the tallest chip with identities has more than ZC_POLY_WAVE_MAX_TERMS = 4,096
    pairs, else zc_poly_wave_kernel (a wave per pair, min(ceil(pairs / 4), 1,024) workgroups of 4 pairs);
  * SP1HIP_ZC_BIVARIATE=0, or one variable: round 0 on base words (zc_macro_kernel<true, KIND>, zc_poly_kernel<true>), round 1
    already on the folded tables.
The reference of the default path is the oracle's `two_round_form` (tests/zc_arbitrary.py says why), that of the sequential path
the plain oracle. SP1HIP_ZC_MUL_MIN_ROWS=1 makes the MulOperation piece run below its default 2^16 rows; the tall Mul cases leave
it at its default."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import pyoracle as orc  # noqa: E402
from kb_edges import EdgeSource  # noqa: E402
from zc_arbitrary import arbitrary_chip, setup  # noqa: E402

KIND_1_2_3, KIND_5, KIND_6 = "Global", "KeccakPermute", "Mul"
# kind 7: two-factor terms, ten identities a row | three-factor terms with selectors | 48 limbs: forms of more than 64 entries, the
# wave form's `k += 64` loop iterates | the modulus comes from memory | a + b + c and a b + c with carry
KIND_7 = ("Secp256k1AddAssign", "Bn254FpOpAssign", "Bls12381FpOpAssign", "Uint256MulMod", "Uint256Ops")
RECURSION = "Poseidon2WideDeg3"          # kind 1 beside preprocessed columns
ALL = (KIND_1_2_3, KIND_5, KIND_6) + KIND_7 + (RECURSION,)
SEQUENTIAL, ONE_STREAM = {"SP1HIP_ZC_BIVARIATE": "0"}, {"SP1HIP_ZC_FORK": "0"}


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _source(kind, seed):
    return np.random.default_rng(seed) if kind == "random" else EdgeSource(seed)


def _first_difference(a, b, L):
    if a == b:
        return "equal"
    if len(a) != len(b):
        return "lengths %d / %d" % (len(a), len(b))
    at = next(k for k in range(len(a)) if a[k] != b[k])
    # (include/sp1hip.h) a u64 count, then 88 bytes per round: a u64 length and five extension coefficients
    return "first differing byte %d of %d (%s)" % (at, len(a), "round %d's message" % ((at - 8) // 88) if 8 <= at < 8 + 88 * L else "behind the round messages")


def _gpu_prove(api, monkeypatch, env, chips, zc, L, seed, zeta, alpha, gkr, publics):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        ch = api.DuplexChallenger()
        ch.observe(orc.random_felts((8,), seed))
        assert np.array_equal(ch.sample_point(L), zeta)
        assert np.array_equal(ch.sample_ext_element(), alpha) and np.array_equal(ch.sample_ext_element(), gkr)
        # (a chip without rows has no tables: tests/test_gpu_zc_real.py)
        up = lambda t: api.ColMajor.from_row_major_host(t) if t is not None and t.shape[0] else None
        dev = [api.ZerocheckChip(air, up(main), up(prep)) for _, air, main, prep in chips]
        blob = api.zerocheck(dev, L, zeta, np.concatenate([c.openings for c in zc]), alpha, gkr, publics, ch)
        return blob, ch.state()


def three_proofs(api, monkeypatch, tables, L, seed, env):
    """tables: [(label, air, main, prep)]. The same tables proved by the oracle (its `two_round_form` on the default path), by the
    pieces and by the interpreter (SP1HIP_ZC_MACRO=0): ((bytes, final transcript state) of each, in that order), and what a
    failure message says about them, or None where all bytes are equal."""
    chips, zc, zeta, alpha, gkr, publics, o_ch = setup(tables, L, seed)
    two_rounds = L >= 2 and env.get("SP1HIP_ZC_BIVARIATE") != "0"
    want = orc.zerocheck_prove(zc, L, zeta, alpha, gkr, publics, o_ch, two_round_form=two_rounds)
    pieces, p_state = _gpu_prove(api, monkeypatch, env, chips, zc, L, seed, zeta, alpha, gkr, publics)
    interp, i_state = _gpu_prove(api, monkeypatch, dict(env, SP1HIP_ZC_MACRO="0"), chips, zc, L, seed, zeta, alpha, gkr, publics)
    differ = None
    if not (pieces == want and interp == want):
        differ = ("pieces vs oracle: %s | interpreter vs oracle: %s | pieces vs interpreter: %s"
                  % (_first_difference(pieces, want, L), _first_difference(interp, want, L), _first_difference(pieces, interp, L)))
    return ((want, o_ch.state()), (pieces, p_state), (interp, i_state)), differ


def check(api, monkeypatch, spec, L, source, seed, env=None, mul_min_rows="1"):
    """spec: [(label, chip, rows)]. Oracle, interpreter (SP1HIP_ZC_MACRO=0) and pieces on the same tables: bytes and transcript."""
    env = dict(env or {})
    if mul_min_rows is not None:
        env["SP1HIP_ZC_MUL_MIN_ROWS"] = mul_min_rows
    src = _source(source, seed)
    tables = [(label,) + arbitrary_chip(chip, rows, src) for label, chip, rows in spec]
    ((_, o_state), (_, p_state), (_, i_state)), differ = three_proofs(api, monkeypatch, tables, L, seed, env)
    if differ:
        pytest.fail("%s, L = %d, %s: %s" % (spec, L, source, differ))
    assert np.array_equal(p_state, o_state), "pieces: transcript state"
    assert np.array_equal(i_state, o_state), "interpreter: transcript state"


# ---- small heights: a missing last row of a pair (has1 false: 1, 3, 5, 7), quads with 1, 2 and 3 live rows (1 | 5, 2 | 6, 3 | 7),
# L = 1: no bivariate rounds (the sequential round 0 on its own), L = 2: the bivariate rounds and nothing behind them
SMALL = [(1, 1), (2, 2), (3, 2), (5, 3), (6, 4), (7, 3)]
SMALL_CASES = [(chip, rows, L) for chip in ALL for rows, L in SMALL if chip != KIND_5 or rows in (1, 3, 6)]     # (Keccak's tables are wide)


@pytest.mark.parametrize("source", ["random", "edge"])
@pytest.mark.parametrize("chip,rows,L", SMALL_CASES, ids=["%s-%d-L%d" % c for c in SMALL_CASES])
def test_small_heights(api, monkeypatch, chip, rows, L, source):
    check(api, monkeypatch, [(chip, chip, rows)], L, source, 100 + rows)


# ---- past one workgroup's share: 1,030 rows = 258 quads in the bivariate kernels and the corner kernel (two workgroups, 256 + 2),
# 129 pairs in round 2; under SP1HIP_ZC_BIVARIATE=0 515 pairs in round 0 (three workgroups, 256 + 256 + 3) and 258 pairs in round 1,
# the first extension round (two workgroups, 256 + 2; the wave form: 65 workgroups, 64 x 4 + 2). Not a multiple of 4: the last quad
# holds two rows. The sequential path's small case: 6 rows.
MID = 1030


@pytest.mark.parametrize("source", ["random", "edge"])
@pytest.mark.parametrize("chip", ALL)
def test_past_one_workgroup(api, monkeypatch, chip, source):
    check(api, monkeypatch, [(chip, chip, MID)], 11, source, 200)


@pytest.mark.parametrize("chip,rows,L,source", [(c, r, lv, s) for c in (KIND_1_2_3, KIND_6, KIND_7[1], KIND_7[2], RECURSION) for r, lv in ((6, 3), (MID, 11)) for s in ("random", "edge")] +
                         [(KIND_5, 6, 3, "random"), (KIND_5, 6, 3, "edge"), (KIND_5, MID, 11, "random")])
def test_sequential_first_rounds(api, monkeypatch, chip, rows, L, source):
    """zc_macro_kernel<true, KIND> and zc_poly_kernel<true> in round 0, the extension forms from round 1 on."""
    check(api, monkeypatch, [(chip, chip, rows)], L, source, 300 + rows, SEQUENTIAL)


def test_one_stream(api, monkeypatch):
    check(api, monkeypatch, [(KIND_1_2_3, KIND_1_2_3, 333), (KIND_7[0], KIND_7[0], 70)], 9, "random", 400, ONE_STREAM)
    check(api, monkeypatch, [(KIND_1_2_3, KIND_1_2_3, 333), (KIND_7[0], KIND_7[0], 70)], 9, "random", 400, dict(SEQUENTIAL, **ONE_STREAM))


# ---- several chips of one kind in one call: one block range and one reduction range per (kind, chip), zc_find_desc searches across
# them; poly_wave is decided by the tallest chip with identities (5,000 rows: 1,250 quads, 625 pairs in round 2) while the shortest
# (3 rows) is down to one pair; two chips with kinds 1, 2, 3 at different heights; Mul beside them through its piece
SEVERAL = [("Bn254FpOpAssign", "Bn254FpOpAssign", 700), ("Global", "Global", 1001), ("Global2", "Global", 6), ("Mul", "Mul", 77),
           ("Poseidon2WideDeg3", "Poseidon2WideDeg3", 130), ("Secp256k1AddAssign", "Secp256k1AddAssign", 3), ("Uint256MulMod", "Uint256MulMod", 5000)]


@pytest.mark.parametrize("env", [{}, SEQUENTIAL], ids=["default", "sequential"])
@pytest.mark.parametrize("source", ["random", "edge"])
def test_several_chips_of_one_kind(api, monkeypatch, source, env):
    check(api, monkeypatch, SEVERAL, 13, source, 500, env)


# ---- the lane / wave switch of the identities. 32,768 rows: 8,192 quads, round 2 has exactly ZC_POLY_WAVE_MAX_TERMS = 4,096 pairs
# and runs the wave form at its cap of 1,024 workgroups x 4 pairs. 32,770 rows: 8,193 rows after the bivariate rounds, 4,097 pairs,
# so round 2 runs zc_poly_kernel<false> (17 workgroups, 16 x 256 + 1) and round 3 the wave form (2,049 pairs, 513 workgroups)
@pytest.mark.parametrize("chip,rows,L,source", [("Bn254FpOpAssign", 32768, 15, "random"), ("Uint256Ops", 32768, 15, "random"),
                                                ("Bn254FpOpAssign", 32770, 16, "random"), ("Uint256Ops", 32770, 16, "random"),
                                                ("Bn254FpOpAssign", 32770, 16, "edge")])
def test_lane_wave_switch_of_the_identities(api, monkeypatch, chip, rows, L, source):
    check(api, monkeypatch, [(chip, chip, rows)], L, source, 600)


# ---- the grid stride of the per-kind kernels, behind min(ceil(terms / 256), 512) workgroups: more than 131,072 terms. Mul (82
# columns; SP1HIP_ZC_MUL_MIN_ROWS at its default, the piece is honoured from 2^16 rows) at 262,146 rows: 131,073 pairs in round 0 of
# the sequential path, where workgroup 0 takes a second pass of one pair. The same table on the default path: 65,537 quads, then
# 32,769 pairs in round 2 (no second pass: the bivariate kernels' own cap is 131,072 QUADS = 524,288 rows, twice what the oracle
# proves in a few seconds; that one form is left to bench.py --full).
@pytest.mark.parametrize("env", [SEQUENTIAL, {}], ids=["sequential", "default"])
def test_grid_stride_of_the_per_kind_kernels(api, monkeypatch, env):
    check(api, monkeypatch, [("Mul", "Mul", 262146)], 19, "random", 700, env, mul_min_rows=None)
