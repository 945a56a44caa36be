"""CPU: the trace checker (sp1_amd/csrc/trace_check.hip) through its host form — tests/native/trace_check runs the __host__
__device__ row functions of sp1_amd/csrc/tc_rows.hpp, the ones the kernels run one row per lane, in a plain loop.

Constraints. For each of the 62 chips of the RISC-V machine and the 8 of the recursion compress machine, 8 arbitrary rows
(zc_arbitrary.arbitrary_chip) from a seeded Generator and from kb_edges.EdgeSource: the value of every constraint on every row is
machine_check.constraint_values' (numpy on the caller's SSA; nothing of the library). Integers, exact equality. KeccakPermute
(2,285 registers by air.allocate_registers) goes through more than one piece; Bls12381DoubleAssign (453) through one; a small
budget cuts a program that fits the default one, with the same values.

Buses. The generalised interaction compiler (lc_compile_interactions, every interaction kept) refuses what lc_compile refuses: a
column outside its table, a constant or weight >= p, a truncated or overlong word list. Over the executed small shard of
tests/lookup_count_cases.py the native messages are exactly machine_check's (kind, values, multiplicity), and the two bucket hashes
are distinct functions: no two distinct messages share their bucket in both tables at log_buckets = 22."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lookup_count_cases as LC  # noqa: E402
import machine_check as MC  # noqa: E402
import pyoracle as orc  # noqa: E402
import trace_check_cases as T  # noqa: E402
from kb_edges import EdgeSource  # noqa: E402
from sp1_amd import air as A  # noqa: E402
from zc_arbitrary import arbitrary_chip, chip_air, publics_read  # noqa: E402

P = T.P
ROWS = 8


@pytest.fixture(scope="module", autouse=True)
def _program():
    assert os.path.exists(T.EXE), "tests/native/trace_check is not built: run __graft_entry__.build()"


def test_the_chip_lists_are_the_machines():
    assert len(T.RISCV) == 62 and len(set(T.RISCV)) == 62 and len(T.RECURSION) == 8


@pytest.mark.parametrize("name", T.RISCV + T.RECURSION)
def test_every_constraint_on_every_row_equals_numpy(name, tmp_path):
    for source in (np.random.default_rng(21), EdgeSource(22)):
        air, main, prep = arbitrary_chip(name, ROWS, source)
        publics = orc.random_felts((publics_read([air]),), 77)
        info, values = T.run_host_air(air, main, prep, publics, tmp_path)
        want = T.host_values(air, main, prep, publics)
        assert values.shape == want.shape == (ROWS, air.num_constraints)
        assert np.array_equal(MC.from_monty(values), want), (name, type(source).__name__)
        if air.num_constraints:
            assert want.any(), "an arbitrary table that violates nothing checks nothing"
            assert info["pieces"] >= 1 and info["registers"] <= 512 and info["lanes"] in (64, 128, 256)
            assert info["registers"] * 4 * info["lanes"] <= 160 * 1024
        else:
            assert info["pieces"] == 0


def test_keccak_is_cut_and_the_largest_program_is_not(tmp_path):
    keccak, bls = chip_air("KeccakPermute"), chip_air("Bls12381DoubleAssign")
    clean = lambda air: np.array([i for i in air.instrs if i[0] != A.HINT], dtype=np.uint32).reshape(-1, 3)
    assert len(bls.instrs) == 72817 and A.allocate_registers(bls.to_array())[1] == 453
    for air, pieces_ok in ((keccak, lambda n: n > 1), (bls, lambda n: n == 1)):
        _, main, prep = arbitrary_chip(air.name, 2, np.random.default_rng(3))
        publics = orc.random_felts((publics_read([air]),), 77)
        info, values = T.run_host_air(air, main, prep, publics, tmp_path)
        assert pieces_ok(info["pieces"]), info
        assert np.array_equal(MC.from_monty(values), T.host_values(air, main, prep, publics))
    # (the hints are pseudo-instructions: the SSA without them is another word list, and no other program)
    assert len(clean(keccak)) < len(keccak.instrs)


@pytest.mark.parametrize("name,budget", [("DivRem", 24), ("Global", 21)])
def test_a_small_budget_cuts_and_changes_no_value(name, budget, tmp_path):
    air, main, prep = arbitrary_chip(name, 5, EdgeSource(9))
    publics = orc.random_felts((publics_read([air]),), 77)
    whole, v0 = T.run_host_air(air, main, prep, publics, tmp_path)
    cut, v1 = T.run_host_air(air, main, prep, publics, tmp_path, max_regs=budget)
    assert whole["pieces"] == 1 and whole["registers"] > budget
    assert cut["pieces"] > 1 and cut["registers"] <= budget
    assert np.array_equal(v0, v1) and np.array_equal(MC.from_monty(v1), T.host_values(air, main, prep, publics))


def test_malformed_programs_are_refused(tmp_path):
    air = chip_air("Add")
    prog = air.to_array().copy()
    main, publics = np.zeros((2, air.main_width), np.uint32), np.zeros(4, np.uint32)
    run = lambda p, w=air.main_width, n=air.num_constraints, pub=publics: T.run_host(p, w, 0, n, main[:, :w], None, pub, tmp_path)
    run(prog)
    first_add = next(k for k, i in enumerate(air.instrs) if i[0] == A.ADD)
    for what, bad in (("column", (prog, air.main_width - 1)), ("count", (prog, air.main_width, air.num_constraints + 1))):
        with pytest.raises(T.Rejected):
            run(*bad)
    forward = prog.copy()
    forward[first_add, 1] = first_add                                  # an operand that is not an earlier value
    opcode = prog.copy()
    opcode[first_add, 0] = 9
    for bad in (forward, opcode):
        with pytest.raises(T.Rejected):
            run(bad)
    reads_public = np.array([[A.PUBLIC, 7, 0], [A.ASSERT_ZERO, 0, 0]], dtype=np.uint32)
    with pytest.raises(T.Rejected):
        T.run_host(reads_public, 1, 0, 1, np.zeros((1, 1), np.uint32), None, publics, tmp_path)


# ---- buses -------------------------------------------------------------------------------------------------------------------------
def _words(it, width=None, prep_width=None):
    return it.to_array(), it.main_width if width is None else width, it.prep_width if prep_width is None else prep_width


def test_the_interaction_compiler_refuses_what_lc_compile_refuses(tmp_path):
    cases = dict(LC.malformed())
    three = cases.pop("three_values")                                  # a byte message of 3 values: the byte counter's rule, not the parser's
    good = LC.message_chip().to_array()
    assert good[5] == 0                                                # [n, is_send, kind, n_values, n_terms, constant, ...]
    constant = good.copy()
    constant[5] = P
    weight = good.copy()
    weight[8] = P                                                      # ... (is_main, column, weight)
    cases.update(constant_at_p=(constant, 6, 0), weight_at_p=(weight, 6, 0))
    for name, (words, main_width, prep_width) in cases.items():
        main = np.zeros((32, main_width), np.int64)
        prep = np.zeros((32, prep_width), np.int64) if prep_width else None
        with pytest.raises(T.Rejected):
            T.run_messages(words, main, prep, tmp_path)
        with pytest.raises(LC.Rejected):                              # ... and so does the byte counter's lc_compile
            LC.run("host", words, np.zeros((main_width, 32), np.uint32), np.zeros((prep_width, 32), np.uint32) if prep_width else None, tmp_path)
    assert len(T.run_messages(three[0], np.ones((4, 6), np.int64), None, tmp_path)) == 4


@pytest.fixture(scope="module")
def shard_messages(tmp_path_factory):
    """[(key, signed multiplicity, hash A, hash B)] of every message of the executed small shard and its public values' row, through
    the native row function; keys from machine_check's own evaluation of the same rows."""
    machine, tabs, _ = LC.shard()
    pv_it, pv_row = LC.public_values_row()
    u64 = lambda t: None if t is None else (t.numpy() if hasattr(t, "numpy") else np.asarray(t)).astype(np.uint64)
    chips = [(it, u64(tabs[name][0]), u64(tabs[name][1])) for name, (_, it) in sorted(machine.items())]
    chips.append((pv_it, None, u64(pv_row).reshape(1, -1)))                       # canonical, like the tables
    out = []
    for it, prep_np, main_np in chips:
        if main_np.shape[0] == 0:
            continue
        got = T.run_messages(it, main_np.astype(np.int64), None if prep_np is None else prep_np.astype(np.int64), tmp_path_factory.mktemp(it.name))
        both = [(1, x) for x in it.sends] + [(-1, x) for x in it.receives]
        want = 0
        for k, (sign, (kind, values, mult)) in enumerate(both):
            m = MC._vcol(mult, prep_np, main_np)
            want += int(np.count_nonzero(m))
            cols = np.stack([MC._vcol(v, prep_np, main_np) for v in values], axis=1) if values else np.zeros((len(m), 0), np.uint64)
            for _, row, mm, is_send, ha, hb in got[got[:, 0] == k].tolist():
                assert mm == int(m[row]) != 0 and is_send == (sign == 1)
                out.append(((kind,) + tuple(int(x) for x in cols[row]), sign * mm, ha, hb))
        assert len(got) == want, it.name
    return chips, out


def test_native_messages_are_machine_checks(shard_messages):
    chips, messages = shard_messages
    assert len(messages) > 11000                                       # 6,759 byte messages sent, one receive per cell they address, every other bus
    tally = {}
    for key, signed, _, _ in messages:
        tally[key] = (tally.get(key, 0) + signed) % P
    assert {k: v for k, v in tally.items() if v} == MC.bus_imbalance(chips) == {}


def test_the_two_bucket_hashes_are_distinct_functions(shard_messages):
    _, messages = shard_messages
    of_key = {}
    for key, _, ha, hb in messages:
        assert of_key.setdefault(key, (ha, hb)) == (ha, hb)            # a function of the message
    keys = list(of_key)
    assert len(keys) > 2000
    for log_buckets in (22, 12):
        a = np.array([of_key[k][0] >> (64 - log_buckets) for k in keys], dtype=np.int64)
        b = np.array([of_key[k][1] >> (64 - log_buckets) for k in keys], dtype=np.int64)
        pairs = a << 32 | b
        if log_buckets == 22:
            assert len(np.unique(pairs)) == len(keys), "two distinct messages share their bucket in both tables"
        else:                                                          # 4,096 buckets: each table collides, the pair of them hardly
            assert len(np.unique(a)) < len(keys) and len(np.unique(b)) < len(keys)
            assert len(keys) - len(np.unique(pairs)) <= 8
            assert np.corrcoef(a, b)[0, 1] < 0.1
