"""CPU: the rows of the Poseidon2 and Uint256MulMod chips and the 512-bit division, as the device kernels compute them, run on the
host. tests/native/p2u_rows (built by __graft_entry__.build()) includes sp1_amd/csrc/tg_poseidon2_rows.hpp and tg_uint256_rows.hpp
unchanged; its `host` form runs the same row functions the kernels of tracegen_poseidon2_uint256.hip call, in a plain loop, and
never opens a GPU.

* the generated events (tests/p2u_cases.py, Python integers) reach what they are meant to: both values of every range-checker bit at
  every position, the pointer and clock edges, all three ways a previous timestamp stands to its access;
* every word of both tables equals the host builders' (poseidon2_shard_from / uint256_shard_from) at every shape of p2u_cases.SHAPES,
  padding rows included;
* the division alone equals Python's divmod on every surviving triple, and divmod with the carry reduced mod 2^256 on two triples
  outside the chip's domain;
* the hash_result columns are the words the events carry, the Uint256MulMod result columns (x y) mod m' computed here;
* the program's widths and column offsets equal R.chip(name)[0].main_width / .layout;
* on the shards of the two hand-assembled programs of tests/test_riscv_exec.py, with the chip's table replaced by the host form's,
  every constraint of every chip vanishes and every bus balances;
* the MemoryLocal records of the two descriptors, through the native memglobal program's host form, are the ones the host shard's
  MemoryLocal rows stand for.
Everything is bit-exact; there are no tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import machine_check as MC  # noqa: E402
import memory_global_cases as G  # noqa: E402
import p2u_cases as C  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(C.EXE), "tests/native/p2u_rows is not built: run __graft_entry__.build()"


def test_the_generated_events_reach_their_cases():
    n, height = C.SHAPES[-1]
    tb = C.host_table("poseidon2", n, height)[:n]
    lay = R.chip("Poseidon2")[0].layout
    for name in ("hash_result_range_checkers", "input_range_checkers"):
        bits = tb[:, lay[name]:lay[name] + 16]
        assert (bits.min(axis=0) == 0).all() and (bits.max(axis=0) == 1).all(), name                  # both values at every position
    first = C.host_table("poseidon2", 32, 32)                                                         # events 1 .. 32 of the list
    assert C.START[32] == 1
    assert (first[0, lay["ptr.addr"] + 1:lay["ptr.addr"] + 3] == 0xFFFF).all() and first[0, lay["ptr.top_two_limb_max.result"]] == 1
    assert len(set(first[1, [lay["addrs.%d.value" % i] + 1 for i in range(8)]].tolist())) == 2        # + 8 i carries into the second limb
    assert set(first[:, lay["clk_low"]].tolist()) >= {0, 1, (1 << 24) - 1}                            # on, above and below a window's start
    for kind, chip, groups in (("poseidon2", "Poseidon2", ["memory.%d" % i for i in range(8)]),
                               ("uint256", "Uint256MulMod", ["%s_memory.%d.memory_access" % (g, i) for g in ("x", "y", "modulus") for i in range(4)])):
        tb, lay = C.host_table(kind, 32, 32), R.chip(chip)[0].layout
        seen = np.concatenate([tb[:, lay[g + ".compare_low"]] for g in groups])
        assert set(seen.tolist()) == {0, 1}, kind                                                     # a previous access in and before the window
        assert any(((tb[:, lay[g + ".diff_low_limb"]] == 0) & (tb[:, lay[g + ".diff_high_limb"]] == 0)).any() for g in groups), kind
    walked = [C.triple_of(r) for n, _ in C.SHAPES for r in C.events("uint256", n)]
    assert len(set(walked)) >= min(len(C.TRIPLES), C.N_EVENTS) - 8 and any(m == 0 for _, _, m in walked) and any(m == 1 for _, _, m in walked)


@pytest.mark.parametrize("kind,n,height", C.KIND_SHAPES)
def test_every_word_equals_the_host_builder(kind, n, height, tmp_path):
    want = C.montgomery_col_major(C.host_table(kind, n, height))
    got = C.run_rows("host", kind, C.events(kind, n), height, tmp_path)
    msg = C.first_difference(kind, want, got, n)
    assert msg is None, msg


def test_more_events_than_rows_are_refused(tmp_path):
    for kind in C.KINDS:
        with pytest.raises(subprocess.CalledProcessError):
            C.run_rows("host", kind, C.events(kind, 33), 32, tmp_path)


def test_the_division_equals_divmod(tmp_path):
    got = C.run_div("host", C.TRIPLES + C.OUTSIDE, tmp_path)
    for (x, y, m), (result, carry) in zip(C.TRIPLES + C.OUTSIDE, got):
        q, r = divmod(x * y, C.modulus_of(m))
        assert (result, carry) == (r, q % C.B256), (hex(x), hex(y), hex(m))
    for (x, y, m), (_, carry) in zip(C.OUTSIDE, got[len(C.TRIPLES):]):
        assert x * y // C.modulus_of(m) >= C.B256 > carry


def test_the_hash_result_columns_are_the_words_written(tmp_path):
    n, height = 65, 96
    ev = C.events("poseidon2", n)
    table = MC.from_monty(C.run_rows("host", "poseidon2", ev, height, tmp_path).T)
    at = R.chip("Poseidon2")[0].layout["hash_result.0"]
    for r in range(n):
        words = [sum(int(table[r, at + 4 * i + k]) << (16 * k) for k in range(4)) for i in range(8)]
        assert words == [int(v) & C.M64 for v in ev[r, 18:26]], r
    assert not table[n:, at:at + 32].any()


def test_the_result_columns_are_the_product_modulo_the_modulus(tmp_path):
    n, height = 300, 320
    ev = C.events("uint256", n)
    table = C.run_rows("host", "uint256", ev, height, tmp_path)
    lay = R.chip("Uint256MulMod")[0].layout
    for r in range(n):
        x, y, m = C.triple_of(ev[r])
        assert C.from_bytes_columns(table, lay["output.result"], r) == x * y % C.modulus_of(m), r
        assert C.from_bytes_columns(table, lay["output.carry"], r) == x * y // C.modulus_of(m), r


def test_widths_and_column_constants_equal_the_transcribed_chips():
    text = subprocess.run([C.EXE, "host", "layout"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, col = line.split()
        air = R.chip(chip)[0]
        assert int(col) == (air.main_width if key == "width" else air.layout[key]), line
        seen.setdefault(chip, set()).add(key)
    assert set(seen) == set(C.CHIPS.values())
    for chip in seen:                                                                                 # every column group is among them
        assert {k.split(".")[0] for k in R.chip(chip)[0].layout} == {k.split(".")[0] for k in seen[chip]} - {"width"}, chip


@pytest.fixture(scope="module")
def program_shards():
    """kind -> (the kind's event records, the host shard) of the hand-assembled program that makes the kind's calls."""
    out = {}
    for kind, (program, _, calls) in C.PROGRAMS.items():
        ex = X.Executor(program(), stdin=[])
        for rec in X.run_records(ex, 1 << 20):
            if rec.kind == kind:
                out[kind] = (np.ascontiguousarray(rec.events), X.host_shard(ex, rec))
        assert kind in out and out[kind][0].shape == (calls, C.WORDS[kind])
    return out


@pytest.mark.parametrize("kind", C.KINDS)
def test_constraints_vanish_and_buses_balance_with_the_host_form_table(kind, program_shards, tmp_path):
    ev, (machine, tables, publics, _) = program_shards[kind]
    chip = C.CHIPS[kind]
    main = tables[chip][1]
    got = C.run_rows("host", kind, ev, int(main.shape[0]), tmp_path)
    msg = C.first_difference(kind, C.montgomery_col_major(main.numpy()), got, len(ev))
    assert msg is None, msg
    tabs = dict(tables)
    tabs[chip] = (tables[chip][0], torch.as_tensor(MC.from_monty(got.T).astype(np.int64)))
    assert tabs[chip][1] is not main
    assert frozenset(a.name for a, _ in machine) in RT.chip_clusters()
    bad, imbalance = MC.check_shard(machine, tabs, publics, PVM.program())
    assert not bad and not imbalance, (bad, imbalance)


@pytest.mark.parametrize("kind", C.KINDS)
def test_constraints_vanish_on_the_generated_satisfying_events(kind, tmp_path):
    """The events of p2u_cases that a run can produce, padding rows included. POSEIDON2: all but every fourth, whose words written
    are not the permutation's. UINT256_MUL: all but those on the last tick of a 2^24 window — x is rewritten at clk_low + 1, which
    the chip states without a carry (a real clock is 1 mod 8 and never stands there); the host builder's table fails there too."""
    n, height = 65, 96
    ev = C.events(kind, n)
    skip = 3 if kind == "poseidon2" else 2
    ev = np.ascontiguousarray(ev[(np.arange(n) + C.START[n]) % 4 != skip])
    air = R.chip(C.CHIPS[kind])[0]
    main = MC.from_monty(C.run_rows("host", kind, ev, height, tmp_path).T)
    cv = MC.constraint_values(air, None, main, np.zeros(X.PV_WORDS, dtype=np.uint64))
    assert cv.shape == (height, air.num_constraints) and not cv.any(), sorted(set(np.argwhere(cv != 0)[:, 1]))[:8]


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", C.SHARD_CALLS)
def test_local_records_equal_the_host_shards(kind, n, tmp_path):
    ev = C.shard_events(kind, n)
    _, tables, _, gev = C.host_shard(kind, n)
    per_call = sum(s[1] for s in C.SEGMENTS[kind])
    ml = tables["MemoryLocal"][1]
    assert ml.shape[0] == RT.pad32(per_call * n) and gev.shape[0] == (2 * per_call + 1) * n
    records = G.run_records(ev, C.SEGMENTS[kind], tmp_path)
    assert records.shape == (per_call * n, 5)
    want = G.local_records_of(ml[:per_call * n])
    assert np.array_equal(records, want), np.argwhere(records != want)[:4]
    args = (C.WORDS[kind],) + C.SYSCALL[kind]
    sp = tables["SyscallPrecompile"][1]
    got = G.run_rows("SyscallPrecompile", ev, int(sp.shape[0]), tmp_path, args)
    msg = G.first_difference("SyscallPrecompile", G.montgomery_col_major(sp), got, n)
    assert msg is None, msg


def test_the_descriptors_are_the_ones_the_api_uses():
    from sp1_amd import api
    assert set(api.WORD_DESCRIPTORS) == set(C.KINDS) == set(X.DEVICE_WORD_KINDS)
    for kind in C.KINDS:
        assert api.WORD_DESCRIPTORS[kind] == (C.WORDS[kind],) + C.SYSCALL[kind] + (C.SEGMENTS[kind],), kind
        chip, control, rows, touched = X.PRECOMPILES[kind]
        assert (chip, control, rows) == (C.CHIPS[kind], None, 1) and touched == sum(s[1] for s in C.SEGMENTS[kind])
