"""The arbitrary tables of tests/zc_arbitrary.py, checked without a GPU: on every chip that tests/test_gpu_zc_pieces.py proves, under
both value sources, the oracle proves, its verifier REJECTS the proof (the tables really violate the constraints: the GPU test does
not compare zeros), a second call gives the same bytes, and every constraint behind a hint is nonzero on at least one of the rows
(through sp1hip_zerocheck_plan_eval, i.e. through the host model of the fused pieces). Also holds the oracle's `two_round_form`:
the same bytes as the plain form on a satisfying trace, other bytes from round 1 on — and only from there — on a table that is not."""
import numpy as np
import pytest

import pyoracle as orc
from kb_edges import EdgeSource
from test_oracle_zerocheck import setup as synthetic_setup
from zc_arbitrary import arbitrary_chip, dead_hinted_constraints, hinted_constraints, setup

# every hint kind: Global 1, 2, 3; KeccakPermute 5; Mul 6; the others 7 (two- and three-factor terms, selectors, 48 limbs, a
# modulus from memory); Poseidon2WideDeg3 (recursion machine, with preprocessed columns) kind 1
CHIPS = ("Global", "KeccakPermute", "Mul", "Secp256k1AddAssign", "Bn254FpOpAssign", "Bls12381FpOpAssign", "Uint256MulMod", "Uint256Ops",
         "Poseidon2WideDeg3")
ROWS, L = 6, 3          # a handful of rows; not a multiple of 4: the last quad holds two real rows


def _source(kind, seed):
    return np.random.default_rng(seed) if kind == "random" else EdgeSource(seed)


@pytest.mark.parametrize("source", ["random", "edge"])
@pytest.mark.parametrize("name", CHIPS)
def test_arbitrary_tables_violate_the_constraints_and_the_oracle_proves_them(name, source):
    air, main, prep = arbitrary_chip(name, ROWS, _source(source, 11))
    assert main.shape == (ROWS, air.main_width) and (prep is None) == (air.prep_width == 0)
    hints = hinted_constraints(air)
    assert hints, name + " carries no hint"
    _, zc, zeta, alpha, gkr, publics, ch = setup({name: (air, main, prep)}, L, 21)
    for two_round_form in (False, True):
        blob = orc.zerocheck_prove(zc, L, zeta, alpha, gkr, publics, ch.clone(), two_round_form=two_round_form)
        assert orc.zerocheck_verify(zc, [ROWS], L, zeta, alpha, gkr, publics, blob, ch.clone()) != 0
        assert orc.zerocheck_prove(zc, L, zeta, alpha, gkr, publics, ch.clone(), two_round_form=two_round_form) == blob
    dead = dead_hinted_constraints(air, main, prep, publics, ROWS)
    assert not dead, (name, source, dead[:8])


def test_two_round_form_changes_nothing_on_a_satisfying_trace():
    for heights, lv in (({"Mul": 5, "Affine": 3, "Sbox": 6}, 3), ({"Affine": 7, "Empty": 0, "Sbox": 2}, 4), ({"Chain": 6, "Manyregs": 5, "Mul": 3}, 3)):
        _, zc, zeta, alpha, gkr, publics, ch = synthetic_setup(heights, lv, 5 + lv)
        plain = orc.zerocheck_prove(zc, lv, zeta, alpha, gkr, publics, ch.clone())
        assert orc.zerocheck_prove(zc, lv, zeta, alpha, gkr, publics, ch.clone(), two_round_form=True) == plain


def test_two_round_form_differs_from_round_1_on_and_not_before():
    """Proof layout (include/sp1hip.h): a u64 count, then per round a u64 length and five extension coefficients (88 bytes a round)."""
    air, main, prep = arbitrary_chip("Mul", ROWS, np.random.default_rng(3))
    _, zc, zeta, alpha, gkr, publics, ch = setup({"Mul": (air, main, prep)}, L, 4)
    plain = orc.zerocheck_prove(zc, L, zeta, alpha, gkr, publics, ch.clone())
    two = orc.zerocheck_prove(zc, L, zeta, alpha, gkr, publics, ch.clone(), two_round_form=True)
    assert len(plain) == len(two) and plain[:8 + 88] == two[:8 + 88] and plain[8 + 88:8 + 2 * 88] != two[8 + 88:8 + 2 * 88]
    # one variable: there is no second round, and the form is the plain one
    _, zc1, zeta1, alpha1, gkr1, publics1, ch1 = setup({"Mul": (air, main[:2], None)}, 1, 4)
    assert orc.zerocheck_prove(zc1, 1, zeta1, alpha1, gkr1, publics1, ch1.clone(), two_round_form=True) == \
        orc.zerocheck_prove(zc1, 1, zeta1, alpha1, gkr1, publics1, ch1.clone())
