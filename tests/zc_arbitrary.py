"""Arbitrary tables of the real chips for the zerocheck (tests/test_zc_arbitrary_host.py, tests/test_gpu_zc_pieces.py,
tests/test_gpu_zc_real.py): no trace generator, no executor, no valid witness. The zerocheck prover is a deterministic function
of whatever tables it is given, and the oracle restates it, so the two are compared byte for byte on tables whose every cell is drawn from a seeded numpy Generator or from
the stored-domain edge pool (tests/kb_edges.py): selectors that are not bits, `is_real` that is not a flag, limbs near p - 1,
constraints that hold nowhere. That is where a wrong term behind a selector, or a wrong coefficient on a column that a satisfying
trace leaves at zero, shows.

What "restates" means on such a table. Every prover leaves the constraints out of node 0 of round 0 (they vanish on real rows; the
reference does the same). The prover of the default path takes rounds 0 AND 1 from one pass over the base tables (zc_biv_*) and
leaves them out of the four Boolean corners of a row quad, i.e. out of node 0 of round 1 as well: `two_round_form` of
`orc.zerocheck_prove` restates that (oracle/kb_zerocheck.hpp). With SP1HIP_ZC_BIVARIATE=0, or one variable, the plain oracle is
the reference."""
import ctypes as C

import numpy as np

import pyoracle as orc
from gkr_real import HEIGHTS
from kb_edges import EdgeSource
from machine_check import constraint_values, from_monty
from sp1_amd import _lib
from sp1_amd import air as A
from sp1_amd.machines import recursion, riscv

P = 0x7F000001
# constraints behind a hint, by kind (sp1_amd/air.py: hint_*; kind 7 carries its own count, kind 8 is an argument of kind 7)
HINT_CONSTRAINTS = {1: 163, 2: 7, 3: 14, 5: 2858, 6: 16}


def chip_air(name):
    """The AirProgram of a chip of the RISC-V machine, or of the recursion machine where the name is one of its chips."""
    for air, _ in recursion.compress_machine():
        if air.name == name:
            return air
    return riscv.chip(name)[0]


def _draw(source, rows, width):
    canonical = np.asarray(source.integers(0, P, size=(rows, width), dtype=np.uint64))
    return orc.to_monty(canonical.astype(np.uint32))


def constraints_of_row(air, main_row, prep_row, publics, form=1):
    """Montgomery words of every constraint on one row (Montgomery words in), the hinted ones through the host model of the fused
    pieces (sp1hip_zerocheck_plan_eval, form 1; `form`: 0 the whole program, 1 chunks, 2 undivided, 3 fine). No GPU involved."""
    lib = _lib.load()
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    prog = np.ascontiguousarray(air.to_array().reshape(-1), dtype=np.uint32)
    out = np.zeros(max(air.num_constraints, 1), dtype=np.uint32)
    m, pub = np.ascontiguousarray(main_row, dtype=np.uint32), np.ascontiguousarray(publics, dtype=np.uint32)
    p = np.ascontiguousarray(prep_row, dtype=np.uint32) if prep_row is not None else np.zeros(1, dtype=np.uint32)
    st = lib.sp1hip_zerocheck_plan_eval(u32p(prog), len(air.instrs), air.main_width, air.prep_width, u32p(m), u32p(p), u32p(pub), len(pub), form,
                                        u32p(out), air.num_constraints, None)
    assert st == 0, lib.sp1hip_last_error().decode()
    return out[:air.num_constraints]


def dead_hinted_constraints(air, main, prep, publics, rows=8):
    """The constraints behind a hint that are zero on every one of the first `rows` rows."""
    live = np.zeros(air.num_constraints, dtype=bool)
    for r in range(min(rows, main.shape[0])):
        live |= constraints_of_row(air, main[r], None if prep is None else prep[r], publics) != 0
    return [k for _, lo, n in hinted_constraints(air) for k in range(lo, lo + n) if not live[k]]


def _main_columns_of(air, asserts, constraint):
    """The main columns a constraint reads (asserts: the instruction index of every ASSERT_ZERO)."""
    cols, seen, stack = set(), set(), [air.instrs[asserts[constraint]][1]]
    while stack:
        k = stack.pop()
        if k in seen:
            continue
        seen.add(k)
        op, a, b = air.instrs[k]
        if op == A.LOAD_MAIN:
            cols.add(a)
        elif op in (A.ADD, A.SUB, A.MUL):
            stack += [a, b]
        elif op == A.NEG:
            stack.append(a)
    return sorted(cols)


def _columns_of(air, asserts, constraint):
    """(main columns, preprocessed columns) a constraint reads, each sorted."""
    main, prep, seen, stack = set(), set(), set(), [air.instrs[asserts[constraint]][1]]
    while stack:
        k = stack.pop()
        if k in seen:
            continue
        seen.add(k)
        op, a, b = air.instrs[k]
        if op == A.LOAD_MAIN:
            main.add(a)
        elif op == A.LOAD_PREP:
            prep.add(a)
        elif op in (A.ADD, A.SUB, A.MUL):
            stack += [a, b]
        elif op == A.NEG:
            stack.append(a)
    return sorted(main), sorted(prep)


_STRUCTURAL = {}


def structurally_zero(air):
    """The constraints that are zero on all 8 rows of one uniform draw (fixed seed; main, preprocessed and public values drawn):
    a nonzero polynomial of these degrees (at most a few hundred, against p = 2^31 - 2^24 + 1) vanishes on 8 independent uniform rows
    with probability below 2^-160, so these are identically zero — x - x, or a product with a constant 0 — and no table makes them
    live. Evaluated by machine_check.constraint_values: numpy on the caller's SSA, nothing of the library under test."""
    if air.name not in _STRUCTURAL:
        rng = np.random.default_rng(0x5A5A)
        main = rng.integers(0, P, size=(8, max(air.main_width, 1)), dtype=np.uint64)
        prep = rng.integers(0, P, size=(8, max(air.prep_width, 1)), dtype=np.uint64)
        publics = rng.integers(0, P, size=publics_read([air]), dtype=np.uint64)
        values = constraint_values(air, prep, main, publics)
        _STRUCTURAL[air.name] = frozenset(int(k) for k in np.nonzero(~values.any(axis=0))[0])
    return _STRUCTURAL[air.name]


def dead_constraints(air, main, prep, publics, rows=64):
    """The constraints outside structurally_zero(air) that are zero on every one of the first `rows` rows of the tables (Montgomery
    words in; a word is zero in either domain or in neither). The same evaluator as structurally_zero."""
    n = min(rows, main.shape[0])
    if n == 0 or air.num_constraints == 0:
        return []
    values = constraint_values(air, None if prep is None else from_monty(prep[:n]), from_monty(main[:n]), from_monty(publics))
    skip = structurally_zero(air)
    return [int(k) for k in np.nonzero(~values.any(axis=0))[0] if int(k) not in skip]


def _repair_all(air, main, prep, rng):
    """arbitrary_chip's loop over dead_constraints: while a constraint outside structurally_zero is zero on every one of the first
    64 rows, one main column that it reads and that has not been redrawn yet (a constant one first) is redrawn uniformly from
    `rng`; a preprocessed column only for a constraint that reads no main column. A dead constraint that reads a column redrawn
    earlier in the same pass waits for the next pass: most of those are live by then, and fewer pool columns are given up. Changes
    main and prep in place; returns the number of redrawn columns. At most 16 passes, then the table is returned as it is (a
    one-row BaseAlu, ExtAlu or PublicValues table cannot be made live at all: tests/test_zc_arbitrary_host.py)."""
    rows = main.shape[0]
    if rows == 0 or air.num_constraints == 0:
        return 0
    publics = orc.random_felts((publics_read([air]),), 77)
    asserts = [k for k, ins in enumerate(air.instrs) if ins[0] == A.ASSERT_ZERO]
    redrawn = {"main": set(), "prep": set()}
    uniform = lambda: orc.to_monty(rng.integers(0, P, size=rows, dtype=np.uint64).astype(np.uint32))
    for _ in range(16):
        dead = dead_constraints(air, main, prep, publics)
        if not dead:
            break
        this_pass, progress = set(), False
        for k in dead:
            main_cols, prep_cols = _columns_of(air, asserts, k)
            kind, table, cols = ("main", main, main_cols) if main_cols else ("prep", prep, prep_cols)
            if any((kind, c) in this_pass for c in cols):
                progress = True
                continue
            fresh = [c for c in cols if c not in redrawn[kind]]
            if not fresh:
                continue
            constant = [c for c in fresh if (table[:, c] == table[0, c]).all()]
            c = (constant or fresh)[0]
            table[:, c] = uniform()
            redrawn[kind].add(c)
            this_pass.add((kind, c))
            progress = True
        if not progress:
            break
    return len(redrawn["main"]) + len(redrawn["prep"])


def arbitrary_chip(name, rows, source, repair="hinted"):
    """(air, main, prep): every main and preprocessed cell drawn from `source` (a seeded numpy Generator or kb_edges.EdgeSource);
    Montgomery words, row-major, `rows` real rows. prep is None for a chip without preprocessed columns.

    An EdgeSource table is made of fifteen words, two fifths of its columns hold one word throughout, and among those words are 0,
    1, -1 and 1/2 (the stored words 0, R1, p - R1 and 0x00ffffff). A constraint that meets the wrong ones is zero on every row, and
    the table is then as blind to it as a satisfying trace. Found on KeccakPermute at 6 rows (2,858 hinted constraints):
      * assert_bool(x) = x (x - 1) of the step_flags / c / a_prime bits whose column holds only 0 and 1, and
        is_real * (computed_index - index) under an all-zero is_real column: 51 constraints;
      * c_prime - xor3(c, c', c'') where one operand and c_prime are whole columns of 1/2 (xor(1/2, y) = 1/2 for every y);
      * d (d - 2)(d - 4), d = the sum of five a_prime bits - c_prime, where six constant columns add up to 0, 2 or 4.
    So, as long as a hinted constraint is zero on every one of the first rows, one main column it reads (a constant one first) is
    redrawn uniformly: random columns are mixed in until no hinted constraint is dead, and every other cell keeps its pool word.

    repair="all" (tests/test_gpu_zc_real.py) asks the same of EVERY constraint, under either source, and returns (air, main, prep,
    the number of redrawn columns): see _repair_all."""
    air = chip_air(name)
    main = _draw(source, rows, air.main_width)
    prep = _draw(source, rows, air.prep_width) if air.prep_width else None
    if repair == "all":
        return air, main, prep, _repair_all(air, main, prep, getattr(source, "rng", source))
    assert repair == "hinted", repair
    rng = getattr(source, "rng", None)
    if rng is not None and rows:
        publics = orc.random_felts((publics_read([air]),), 77)
        asserts = [k for k, ins in enumerate(air.instrs) if ins[0] == A.ASSERT_ZERO]
        for _ in range(16):
            dead = dead_hinted_constraints(air, main, prep, publics)
            if not dead:
                break
            for k in dead:
                cols = _main_columns_of(air, asserts, k)
                constant = [c for c in cols if (main[:, c] == main[0, c]).all()]
                c = (constant or cols)[0]
                main[:, c] = orc.to_monty(rng.integers(0, P, size=rows, dtype=np.uint64).astype(np.uint32))
    return air, main, prep


def hinted_constraints(air):
    """[(hint kind, first constraint, number of constraints)] of the hints an AirProgram carries, in program order."""
    out, asserts = [], 0
    for op, a, b in air.instrs:
        if op == A.ASSERT_ZERO:
            asserts += 1
        elif op == A.HINT and (a & 0xFF) != 8:
            kind = a & 0xFF
            out.append((kind, asserts, b if kind == 7 else HINT_CONSTRAINTS[kind]))
    return out


def publics_read(airs):
    """How many public values the programs read: one past the largest index of a PUBLIC instruction (at least 2, as the synthetic
    AIRs' set-up passes; SyscallInstrs reads 148)."""
    n = 2
    for air in airs:
        n = max([n] + [a + 1 for op, a, _ in air.instrs if op == A.PUBLIC])
    return n


def setup(chips, L, seed):
    """chips: {name: (air, main, prep)} or [(name, air, main, prep)]. The transcript prologue of tests/test_oracle_zerocheck.py::setup
    (observe eight seeded felts, sample zeta, then alpha and gkr). Returns (chips in name order — the order of the reference's
    BTreeMap, which the shard prover hands to the zerocheck —, the orc.ZcChip list with padded_column_openings, zeta, alpha, gkr,
    publics, the oracle challenger)."""
    if isinstance(chips, dict):
        chips = [(name,) + tuple(v) for name, v in chips.items()]
    chips = sorted(chips, key=lambda c: c[0])
    publics = orc.random_felts((publics_read([c[1] for c in chips]),), seed + 1000)
    ch = orc.Challenger()
    ch.observe(orc.random_felts((8,), seed))
    zeta = ch.sample_point(L)
    alpha, gkr = ch.sample_ext(), ch.sample_ext()
    zc = []
    for name, air, main, prep in chips:
        op = [orc.padded_column_openings(main, L, zeta)]
        if prep is not None:
            op.append(orc.padded_column_openings(prep, L, zeta))
        zc.append(orc.ZcChip(air.to_array(), air.main_width, air.prep_width, air.num_constraints, main, prep, np.concatenate(op)))
    return chips, zc, zeta, alpha, gkr, publics, ch


# ---- the cases of tests/test_gpu_zc_real.py: every real chip's program on tables that violate it, repair="all" ------------------------
# (kept here so that tests/test_zc_arbitrary_host.py can hold, without a GPU, that these very tables are live)
CORE = sorted(riscv.CHIPS)                                                          # 30 chips, 27 of them with constraints
REST =["AluX0", "DivRem", "KeccakPermuteControl", "MemoryGlobalFinalize", "MemoryGlobalInit", "ShaCompress", "ShaCompressControl",
        "ShaExtend", "ShaExtendControl", "SyscallCore", "SyscallInstrs", "SyscallPrecompile"]       # MORE_CHIPS without a hint
RECURSION = [air.name for air, _ in recursion.compress_machine()]
# hinted chips that no other GPU test proves on violating tables (tests/test_gpu_zc_pieces.py::ALL has the other ten)
UNPROVED = ["Bls12381AddAssign", "Bls12381DoubleAssign", "Bls12381Fp2AddSubAssign", "Bls12381Fp2MulAssign", "Bn254AddAssign",
            "Bn254DoubleAssign", "Bn254Fp2AddSubAssign", "Bn254Fp2MulAssign", "EdAddAssign", "EdDecompress", "Poseidon2",
            "Secp256k1DoubleAssign", "Secp256r1AddAssign", "Secp256r1DoubleAssign"]
PIECES_ALL = ["Global", "KeccakPermute", "Mul", "Secp256k1AddAssign", "Bn254FpOpAssign", "Bls12381FpOpAssign", "Uint256MulMod", "Uint256Ops",
              "Poseidon2WideDeg3"]
# ZcPlan::mono / chunks / fine: the six un-hinted programs with the most to lose from a mis-cut chunk, and the two programs
# (Global, Poseidon2: through the interpreter, SP1HIP_ZC_MACRO=0) that plan_round runs undivided (tests/test_gpu_zc_real.py)
FORMS = ["Branch", "ShiftRight", "DivRem", "KeccakPermuteControl", "ShaCompress", "SyscallInstrs", "Global", "Poseidon2"]
FORMS_ROWS, FORMS_L = 8198, 14


def _cycled(names, shift):
    return [(n, n, HEIGHTS[(i + shift) % len(HEIGHTS)]) for i, n in enumerate(names)]


# name -> (spec [(label, chip, rows)], L, source kind, seed)
REAL_CASES = {
    "core-rand": (_cycled(CORE, 0), 8, "random", 31), "core-edge": (_cycled(CORE, 5), 8, "edge", 32),
    "rest-rand": (_cycled(REST, 2), 8, "random", 33), "rest-edge": (_cycled(REST, 9), 8, "edge", 34),
    "recursion-rand": (_cycled(RECURSION, 3), 8, "random", 35), "recursion-edge": (_cycled(RECURSION, 14), 8, "edge", 40),
    "forms-rand": ([(n, n, FORMS_ROWS) for n in FORMS], FORMS_L, "random", 37),
    "forms-edge": ([(n, n, FORMS_ROWS) for n in FORMS], FORMS_L, "edge", 38),
}
for _n in UNPROVED:
    for _kind, _s in (("random", 41), ("edge", 42)):
        REAL_CASES["%s-5-%s" % (_n, _kind)] = ([(_n, _n, 5)], 3, _kind, _s)
        REAL_CASES["%s-130-%s" % (_n, _kind)] = ([(_n, _n, 130)], 8, _kind, _s + 2)
for _n in PIECES_ALL:
    REAL_CASES["%s-6-edge" % _n] = ([(_n, _n, 6)], 3, "edge", 45)
    REAL_CASES["%s-130-edge" % _n] = ([(_n, _n, 130)], 8, "edge", 46)

_real = {}


def real_case(name):
    """(tables [(label, air, main, prep)], redrawn columns per table, L, seed): made once per name and shared, never changed."""
    if name not in _real:
        spec, L, kind, seed = REAL_CASES[name]
        src = np.random.default_rng(seed) if kind == "random" else EdgeSource(seed)
        made = [(label,) + arbitrary_chip(chip, rows, src, repair="all") for label, chip, rows in spec]
        assert all(t[2].shape[0] <= 1 << L for t in made)
        _real[name] = ([t[:4] for t in made], [t[4] for t in made], L, seed)
    return _real[name]
