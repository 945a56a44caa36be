"""The arbitrary tables of tests/zc_arbitrary.py, checked without a GPU: on every chip that tests/test_gpu_zc_pieces.py proves, under
both value sources, the oracle proves, its verifier REJECTS the proof (the tables really violate the constraints: the GPU test does
not compare zeros), a second call gives the same bytes, and every constraint behind a hint is nonzero on at least one of the rows
(through sp1hip_zerocheck_plan_eval, i.e. through the host model of the fused pieces). Also holds the oracle's `two_round_form`:
the same bytes as the plain form on a satisfying trace, other bytes from round 1 on — and only from there — on a table that is not.

repair="all" (the tables of tests/test_gpu_zc_real.py). The loop above repairs hinted constraints only, and a constraint without a
hint can be just as dead on an EdgeSource table: at 130 rows 20 of ShiftRight's 78, 3 of SyscallInstrs' 93, 6 of DivRem's 348, 160 of
KeccakPermute's 2,859, 7 to 15 of every curve chip's are zero on every row before the repair. So for every one of the 70 chips (30
of riscv.CHIPS, 32 of riscv_more.MORE_CHIPS, 8 of the recursion machine), both sources, 6 and 130 rows:
  * no constraint outside `structurally_zero` is dead (machine_check.constraint_values: numpy on the SSA, nothing of the library);
  * at most a third of the main columns were redrawn, so an edge table is still an edge table. Seen with these seeds (source seed
    5 + rows), at 6 / 130 rows: a Generator table is never repaired; of EdgeSource tables SyscallInstrs 0 / 4 of 65 columns (6.2 %),
    KeccakPermute 52 / 160 of 2,640 (6.1 %), ShiftRight 0 / 4 of 69 (5.8 %), MemoryLocal 0 / 1 of 20, ShaCompress 10 / 2 of 206
    (4.9 %), Lt 0 / 2 of 44, DivRem 2 / 7 of 246 (2.8 %), every curve and tower chip at most 2.0 % (Bls12381FpOpAssign 9 of 450,
    Secp256r1AddAssign 22 of 1,599); 37 of the 70 chips keep every column. The recursion machine's BaseAlu, ExtAlu and
    PublicValues (3, 12 and 1 main columns behind 8 to 10 preprocessed selectors and addresses) are live as drawn on about half
    of all seeds and beyond repair through main columns on the others — a selector column that holds stored 0 on the first 64 rows
    kills its constraints whatever the main columns hold — which is why the seed is chosen;
  * the oracle proves them in both forms, its verifier rejects both (status 2: the claimed evaluation is not the constraints' at
    the point), a second call gives the same bytes. Byte, Program, Range, MemoryConst and MemoryVar have no constraints: nothing
    can be violated, both forms give the same bytes and the verifier ACCEPTS (status 0);
  * forms 0 to 3 of sp1hip_zerocheck_plan_eval give what constraint_values gives on the first three rows of the table: stored 0,
    R1, p - R1 and 0x00ffffff are the words that immediate folding and the RSUB / MADC rewrites treat specially, and
    tests/test_zc_compiler.py draws uniform rows only.
Constraints that are zero whatever the table holds (`structurally_zero`, pinned per chip below): 29 of DivRem, 16 of ShaCompress, 64
of Poseidon2, 3 each of LoadDouble, StoreDouble and Lt, 2 each of LoadWord and StoreWord, 1 each of LoadHalf, StoreHalf, UType,
MemoryLocal, MemoryGlobalInit, MemoryGlobalFinalize, SyscallCore, SyscallPrecompile and Poseidon2WideDeg3; none anywhere else.
The tables of the GPU cases themselves (zc_arbitrary.REAL_CASES) are held to the same two conditions wherever they have 5 rows or
more; the 22 shorter ones of the cycled heights (1 to 4 rows; 12 of them EdgeSource) are exempt from both — a one-row table of
BaseAlu, ExtAlu or PublicValues cannot be made live through main columns — and the number of dead constraints seen on them is
recorded as an assertion: 0 on all 22 with the seeds chosen, after 8 of SyscallInstrs' 65 columns were redrawn at 2 rows, 3 of
LoadX0's 48 at 1 row, one each of Lt's and PrefixSumChecks', and none elsewhere."""
import numpy as np
import pytest

import pyoracle as orc
from kb_edges import EdgeSource
from test_oracle_zerocheck import setup as synthetic_setup
from machine_check import constraint_values, from_monty
from sp1_amd.machines import recursion, riscv
from sp1_amd.machines.riscv_more import MORE_CHIPS
from zc_arbitrary import (REAL_CASES, arbitrary_chip, chip_air, constraints_of_row, dead_constraints, dead_hinted_constraints, hinted_constraints,
                          publics_read, real_case, setup, structurally_zero)

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


# ---- repair="all": every chip, every constraint ---------------------------------------------------------------------------------------
EVERY_CHIP = sorted(riscv.CHIPS) + sorted(MORE_CHIPS) + [air.name for air, _ in recursion.compress_machine()]
NO_CONSTRAINTS = ("Byte", "Program", "Range", "MemoryConst", "MemoryVar")
STRUCTURALLY_ZERO = {"DivRem": 29, "ShaCompress": 16, "Poseidon2": 64, "LoadDouble": 3, "StoreDouble": 3, "Lt": 3, "LoadWord": 2, "StoreWord": 2,
                     "LoadHalf": 1, "StoreHalf": 1, "UType": 1, "MemoryLocal": 1, "MemoryGlobalInit": 1, "MemoryGlobalFinalize": 1,
                     "SyscallCore": 1, "SyscallPrecompile": 1, "Poseidon2WideDeg3": 1}
ALL_SEED = 5            # source seed ALL_SEED + rows (see the module docstring: the recursion chips are why it is chosen)


def test_there_are_seventy_chips():
    assert len(EVERY_CHIP) == len(set(EVERY_CHIP)) == 70 and (len(riscv.CHIPS), len(MORE_CHIPS)) == (30, 32)
    assert sorted(n for n in EVERY_CHIP if chip_air(n).num_constraints == 0) == sorted(NO_CONSTRAINTS)


def test_structurally_zero_counts_are_pinned():
    """A count that changes is a finding about the transcription of that chip, not something to absorb."""
    assert {n: len(structurally_zero(chip_air(n))) for n in EVERY_CHIP if structurally_zero(chip_air(n))} == STRUCTURALLY_ZERO
    # ... and they are zero on another draw as well, with other public values
    rng = np.random.default_rng(9)
    for name in STRUCTURALLY_ZERO:
        air = chip_air(name)
        main = rng.integers(0, 0x7F000001, size=(4, air.main_width), dtype=np.uint64)
        prep = rng.integers(0, 0x7F000001, size=(4, max(air.prep_width, 1)), dtype=np.uint64)
        values = constraint_values(air, prep, main, rng.integers(0, 0x7F000001, size=publics_read([air]), dtype=np.uint64))
        assert not values[:, sorted(structurally_zero(air))].any(), name


@pytest.mark.parametrize("rows,lv", [(6, 3), (130, 8)])
@pytest.mark.parametrize("source", ["random", "edge"])
@pytest.mark.parametrize("name", EVERY_CHIP)
def test_every_constraint_of_every_chip_is_live_after_repair_all(name, source, rows, lv):
    air, main, prep, redrawn = arbitrary_chip(name, rows, _source(source, ALL_SEED + rows), repair="all")
    assert main.shape == (rows, air.main_width) and (prep is None) == (air.prep_width == 0)
    _, zc, zeta, alpha, gkr, publics, ch = setup({name: (air, main, prep)}, lv, 21)
    dead = dead_constraints(air, main, prep, publics)
    assert not dead, (name, source, rows, len(dead), dead[:8])
    assert 3 * redrawn <= air.main_width, (name, source, rows, redrawn, air.main_width)
    assert source == "edge" or redrawn == 0
    blobs = []
    for two_round_form in (False, True):
        blob = orc.zerocheck_prove(zc, lv, zeta, alpha, gkr, publics, ch.clone(), two_round_form=two_round_form)
        status = orc.zerocheck_verify(zc, [rows], lv, zeta, alpha, gkr, publics, blob, ch.clone())
        assert status == (0 if name in NO_CONSTRAINTS else 2), (name, two_round_form, status)
        assert orc.zerocheck_prove(zc, lv, zeta, alpha, gkr, publics, ch.clone(), two_round_form=two_round_form) == blob
        blobs.append(blob)
    assert (blobs[0] == blobs[1]) == (name in NO_CONSTRAINTS)
    # the compiler's four forms on the first three rows of this table
    want = constraint_values(air, None if prep is None else from_monty(prep[:3]), from_monty(main[:3]), from_monty(publics))
    for row in range(3 if air.num_constraints else 0):
        for form in range(4):
            got = from_monty(constraints_of_row(air, main[row], None if prep is None else prep[row], publics, form))
            assert np.array_equal(got, want[row]), (name, source, row, form, np.nonzero(got != want[row])[0][:8])


@pytest.mark.parametrize("case", sorted(REAL_CASES))
def test_the_tables_of_the_gpu_cases_are_live(case):
    tables, redrawn, lv, seed = real_case(case)
    publics = orc.random_felts((publics_read([t[1] for t in tables]),), seed + 1000)         # (what `setup` passes)
    for (label, air, main, prep), n in zip(tables, redrawn):
        dead = dead_constraints(air, main, prep, publics)
        assert not dead, (case, label, main.shape[0], len(dead), dead[:8])
        if main.shape[0] >= 5:
            assert 3 * n <= air.main_width, (case, label, main.shape[0], n, air.main_width)


def test_the_gpu_cases_prove_every_chip():
    from zc_arbitrary import CORE, PIECES_ALL, RECURSION, REST, UNPROVED
    assert (len(CORE), len(REST), len(RECURSION), len(UNPROVED), len(PIECES_ALL)) == (30, 12, 8, 14, 9)
    assert tuple(PIECES_ALL[:3] + PIECES_ALL[-1:]) == ("Global", "KeccakPermute", "Mul", "Poseidon2WideDeg3") and all(hinted_constraints(chip_air(n)) for n in UNPROVED + PIECES_ALL)
    assert not any(hinted_constraints(chip_air(n)) for n in REST)
    proved = {chip for spec, _, _, _ in REAL_CASES.values() for _, chip, _ in spec}
    assert proved == set(EVERY_CHIP)
