"""GPU parity (-m gpu) of the zerocheck on EVERY real chip's constraint program, on tables that violate it: the 30 chips of
riscv.CHIPS, the 32 of riscv_more.MORE_CHIPS and the 8 of the recursion machine. tests/test_gpu_zc_pieces.py proves nine of them on
such tables (one per hint kind, to pin the fused pieces); every other program reached the GPU only inside whole-shard proofs of
satisfying traces, where every constraint is zero on every row, selectors are 0 or 1, limbs are bytes and padding is is_real = 0:
there a wrong coefficient, a clobbered register or a mis-cut chunk of the interpreter kernels (zc_round_kernel,
zc_biv_round_kernel, zc_biv_corner_kernel) gives the same all-zero sums. Every case here proves the same tables three times —
oracle (`two_round_form` on the default path, the plain form under SP1HIP_ZC_BIVARIATE=0), fused pieces, interpreter
(SP1HIP_ZC_MACRO=0) — and compares proof bytes and the final transcript state; no tolerance anywhere. The tables are
zc_arbitrary.REAL_CASES, made with repair="all": tests/test_zc_arbitrary_host.py holds without a GPU that every constraint that can
be nonzero is nonzero on some row of every one of them. Chips go in name order, as `setup` sorts them. When a case of several chips
differs, every chip is proved once more on its own and the failure names those whose bytes differ.

The cases, and what plan_round (sp1_amd/csrc/zerocheck.hip) makes of them. Heights "cycled" are gkr_real.HEIGHTS (0 .. 9, 12, 37,
64, 111, 130, 255, 256: every quad residue, zero-row chips, one tile and one row less) dealt round the chips from two shifts.
  * core-rand / core-edge: the 30 core chips in one call, L = 8 — 27 programs in one launch beside three chips that have
    preprocessed columns and no constraints (Byte, Program, Range); default path, SP1HIP_ZC_BIVARIATE=0 and SP1HIP_ZC_FORK=0.
  * rest-rand / rest-edge: the 12 chips of MORE_CHIPS without a hint (SyscallInstrs reads 148 public values); both paths.
  * recursion-rand / recursion-edge: the 8 chips of the compress machine, all with preprocessed columns, two without constraints,
    Poseidon2WideDeg3 through its piece beside them.
  * the 14 hinted chips that no test proved on violating tables (zc_arbitrary.UNPROVED), each alone at 5 rows (L = 3) and 130
    rows (L = 8), both sources: their 300 to 400 un-hinted constraints (24 to 51 chunks beside the identities) and, on the
    interpreter's leg, the longest programs there are (Bls12381DoubleAssign: 72,817 SSA instructions, 97,673 words in 937 chunks).
  * the nine chips of test_gpu_zc_pieces.py::ALL once more with repair="all", EdgeSource, 6 and 130 rows: that file's tables keep
    only the hinted constraints live.
  * forms: Branch, ShiftRight, DivRem, KeccakPermuteControl, ShaCompress, SyscallInstrs, and Global and Poseidon2, in one call at
    8,198 rows, L = 14. Confirmed from plan_round and the plans (sizes below): the default path has 2,050 quads in the bivariate
    kernels, then 1,025, 513, 257, 129 and 65 pairs in rounds 2 to 6 and 33 .. 1 in rounds 7 to 13; SP1HIP_ZC_BIVARIATE=0 has 4,099
    pairs of base words in round 0 and 2,050 in round 1. A program runs UNDIVIDED (ZcPlan::mono) from ZC_MONO_MIN_TERMS = 1,024 terms
    only if its chunks hold more than 1.5 times the words of the undivided form, and not one of the 65 programs planned with hints
    does (DivRem: 3,891 against 3,565 words): the six un-hinted chips run CHUNKED down to 65 pairs and FINE from 33
    pairs (ZC_FINE_MAX_TERMS = 64) on both legs. The only real programs that take the undivided form are Global (8,316 words in 47
    chunks against 4,993) and Poseidon2 (9,586 in 64 against 6,109) with their hints ignored, i.e. on the interpreter's leg of this
    case — in the bivariate kernels and round 2 of the default path, rounds 0 to 2 of the sequential one — which is why the two are
    in it. Without them ZcPlan::mono is run by the synthetic AIRs of tests/test_gpu_zerocheck.py alone.
  * LDS staging: core-rand and rest-rand under SP1HIP_ZC_STAGE_MAX=1024 and =32. No piece of any form of any real program is
    longer than 517 instructions (chunks at most 320 but for single constraints' cones: Bls12381FpOpAssign 517, EdAddAssign 460;
    Global without hints 396), so 1,024 stages EVERYTHING; at these heights (at most 64 quads) plan_round picks the fine cut, whose
    largest pieces are at most 32 instructions for most chips and 37 (LoadX0, ShaCompress), 38 (Sub), 54 (SyscallInstrs), 72 (Mul
    without its hint), 97 (DivRem) and 396 (Global without hints): under 32 both fetch paths run in one round, in two launches
    (a group is (staged, workgroup width, resident workgroups)).

Registers and the workgroup width. zc_wg_for picks, among 256, 128 and 64 lanes, the width that keeps most lanes resident beside
an LDS register file of 16 bytes a lane and register (extension rounds and the bivariate kernels): 256 lanes for 1 to 4, 13, 18, 19
and 32 to 39 registers, 128 for 6, 7, 11, 15 and 23 to 26, 64 for 5, 8 to 10, 12, 14, 16, 17, 20 to 22, 27 to 31 and from 40 on; none
(the fine cut instead) above 160. The largest file over the pieces of the CHUNKED form, from sp1hip_zerocheck_plan_eval's stats and
the plans, with hints honoured:
  * 256 lanes: Bitwise, StateBump, Select, Poseidon2 and every curve and tower chip but EdDecompress (4 registers each), PublicValues
    (2), MemoryLocal, SyscallCore, SyscallPrecompile, KeccakPermute, Poseidon2WideDeg3 (1), MemoryGlobalInit / Finalize (13),
    ShiftRight (19);
  * 128 lanes: Add, Addi, Addw, Sub, Jalr, LoadDouble, StoreDouble, StoreHalf, BaseAlu (7), Subw, StoreWord, MemoryBump, Global (6),
    LoadHalf (11), SyscallInstrs (23);
  * 64 lanes: AluX0, DivRem, ShaCompressControl, ShaExtendControl, Uint256MulMod (5), UType (8), Jal, KeccakPermuteControl (9),
    LoadWord, EdDecompress (10), LoadByte, StoreByte, ShaExtend, Uint256Ops, PrefixSumChecks (12), LoadX0, Mul (14), Lt, ShiftLeft,
    ExtAlu (16), Branch (17), ShaCompress (28).
With hints ignored (the interpreter's leg): 256 lanes for Bn254FpOpAssign (19), Uint256Ops (18), KeccakPermute (32), Uint256MulMod
(34) and the Add / Fp2 chips that stay at 4; 128 for EdDecompress, Secp256k1DoubleAssign and Secp256r1DoubleAssign (11); 64 for
Bn254DoubleAssign (10), Bls12381DoubleAssign (14), Global and Poseidon2WideDeg3 (20), Bls12381FpOpAssign and Mul (27), Poseidon2
(31), Bls12381Fp2AddSubAssign and EdAddAssign (5). The fine cuts move chips between tiers (ShaCompress and SyscallInstrs 18: 256;
Branch, Lt, ShiftLeft 11: 128; ShiftRight 10: 64), the undivided forms of Global (23: 128) and Poseidon2 (31: 64) are the ones the
forms case runs. In round 0 of the sequential path a register is 4 bytes and a chunked program of up to 19 registers gets 256
lanes: the first narrower width comes at 20 registers, which only ShaCompress (28: 128),
SyscallInstrs (23: 64) and, without hints, Global (20: 64), Mul and Bls12381FpOpAssign (27: 64), Poseidon2 (31: 256), KeccakPermute
(32: 64) and Uint256MulMod (34: 128) reach. So every tier of either rule is reached by real programs. No real program has a form
whose file does not fit (KeccakPermute's undivided form without its hint would take 643 registers and is refused for the undivided
form before that matters): the fall-back from wg = 0 to the fine cut stays with the synthetic Manyregs AIR of
tests/test_gpu_zerocheck.py.

Wall time of this file on an MI355X: see DESIGN.md §11.0.5."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import zc_arbitrary as ZA  # noqa: E402
from test_gpu_zc_pieces import ALL, ONE_STREAM, SEQUENTIAL, api, three_proofs  # noqa: E402,F401  (api: the fixture)

STAGE_ALL, STAGE_SOME = {"SP1HIP_ZC_STAGE_MAX": "1024"}, {"SP1HIP_ZC_STAGE_MAX": "32"}


def run_case(api, monkeypatch, name, env=None):
    tables, _, L, seed = ZA.real_case(name)
    env = dict(env or {}, SP1HIP_ZC_MUL_MIN_ROWS="1")           # (Mul's piece below its default 2^16 rows, as in test_gpu_zc_pieces.py)
    ((_, o_state), (_, p_state), (_, i_state)), differ = three_proofs(api, monkeypatch, tables, L, seed, env)
    if differ:
        alone = []
        if len(tables) > 1:
            for t in tables:
                if t[2].shape[0]:
                    _, d = three_proofs(api, monkeypatch, [t], L, seed, env)
                    if d:
                        alone.append("%s (%d rows): %s" % (t[0], t[2].shape[0], d))
            differ += " || chips that differ when proved alone: " + ("; ".join(alone) if alone else "none (only together)")
        pytest.fail("%s, L = %d, %s: %s" % (name, L, env, differ))
    assert np.array_equal(p_state, o_state), "pieces: transcript state"
    assert np.array_equal(i_state, o_state), "interpreter: transcript state"


@pytest.mark.parametrize("env", [{}, SEQUENTIAL, ONE_STREAM], ids=["default", "sequential", "one-stream"])
@pytest.mark.parametrize("case", ["core-rand", "core-edge"])
def test_the_thirty_core_chips_in_one_call(api, monkeypatch, case, env):
    run_case(api, monkeypatch, case, env)


@pytest.mark.parametrize("env", [{}, SEQUENTIAL], ids=["default", "sequential"])
@pytest.mark.parametrize("case", ["rest-rand", "rest-edge", "recursion-rand", "recursion-edge"])
def test_the_unhinted_chips_and_the_recursion_machine(api, monkeypatch, case, env):
    run_case(api, monkeypatch, case, env)


@pytest.mark.parametrize("source", ["random", "edge"])
@pytest.mark.parametrize("rows", [5, 130])
@pytest.mark.parametrize("chip", ZA.UNPROVED)
def test_the_hinted_chips_nobody_proved_on_violating_tables(api, monkeypatch, chip, rows, source):
    run_case(api, monkeypatch, "%s-%d-%s" % (chip, rows, source))


@pytest.mark.parametrize("rows", [6, 130])
@pytest.mark.parametrize("chip", ALL)
def test_the_chips_of_the_pieces_with_every_constraint_live(api, monkeypatch, chip, rows):
    run_case(api, monkeypatch, "%s-%d-edge" % (chip, rows))


@pytest.mark.parametrize("env", [{}, SEQUENTIAL], ids=["default", "sequential"])
@pytest.mark.parametrize("case", ["forms-rand", "forms-edge"])
def test_the_three_forms_of_a_program(api, monkeypatch, case, env):
    """8,198 rows: undivided (Global and Poseidon2 on the interpreter's leg), chunked and fine forms in one proof (module docstring)."""
    run_case(api, monkeypatch, case, env)


@pytest.mark.parametrize("env", [STAGE_ALL, STAGE_SOME], ids=["stage-1024", "stage-32"])
@pytest.mark.parametrize("case", ["core-rand", "rest-rand"])
def test_programs_staged_in_lds(api, monkeypatch, case, env):
    run_case(api, monkeypatch, case, env)
