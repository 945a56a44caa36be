"""Arbitrary tables of the real chips for the zerocheck (tests/test_zc_arbitrary_host.py, tests/test_gpu_zc_pieces.py): no trace
generator, no executor, no valid witness. The zerocheck prover is a deterministic function of whatever tables it is given, and the
oracle restates it, so the two are compared byte for byte on tables whose every cell is drawn from a seeded numpy Generator or from
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


def constraints_of_row(air, main_row, prep_row, publics):
    """Montgomery words of every constraint on one row (Montgomery words in), the hinted ones through the host model of the fused
    pieces (sp1hip_zerocheck_plan_eval, form 1). No GPU involved."""
    lib = _lib.load()
    u32p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    prog = np.ascontiguousarray(air.to_array().reshape(-1), dtype=np.uint32)
    out = np.zeros(max(air.num_constraints, 1), dtype=np.uint32)
    m, pub = np.ascontiguousarray(main_row, dtype=np.uint32), np.ascontiguousarray(publics, dtype=np.uint32)
    p = np.ascontiguousarray(prep_row, dtype=np.uint32) if prep_row is not None else np.zeros(1, dtype=np.uint32)
    st = lib.sp1hip_zerocheck_plan_eval(u32p(prog), len(air.instrs), air.main_width, air.prep_width, u32p(m), u32p(p), u32p(pub), len(pub), 1,
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


def arbitrary_chip(name, rows, source):
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
    redrawn uniformly: random columns are mixed in until no hinted constraint is dead, and every other cell keeps its pool word."""
    air = chip_air(name)
    main = _draw(source, rows, air.main_width)
    prep = _draw(source, rows, air.prep_width) if air.prep_width else None
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
