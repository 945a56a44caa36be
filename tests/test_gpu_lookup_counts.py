"""GPU (-m gpu): the Byte, Range and Program multiplicities counted on the device (sp1hip_lookup_count_sends / _count_program /
_counts_finish through api.LookupCounter and riscv_exec.device_lookup_tables) against the host tracer's count, whole tables, word for
word. The synthetic one-send chips of tests/lookup_count_cases.py at heights 1, 63, 64, 65, 257 — lanes that share a cell with
different multiplicities among them — and every row on one cell at 65,537 rows (257 workgroups, still ONE pass of the grid); tables and
a list of pcs of 2048 * 256 + 257 rows, more than a pass of the 2,048-workgroup grid holds, so that the grid stride runs and ends
inside a workgroup: every row on one cell, and runs of three rows per cell with multiplicities 1, 2, 1, 2, ...; a finished counter
refuses further calls; a counter on a stream of its own; the native program's device form
against its host form, which tests/test_lookup_counts_host.py pins to the tracer on the CPU, on every chip of the generated shard; a
bad message is an Sp1HipError that names its send and row and leaves the good messages' counts as they are (an ordinary error
return: the kernel checks before it indexes); the corner programs of riscv_row_cases / riscv_mem_row_cases from staged host tables
and from core_device_tables, Program from device and from host events; the clock-window tables; a one-event Keccak precompile shard;
and a small program proved from host tables, with the 23 chips' tables device-made, and with device-counted Byte, Range and Program
as well: the same proof bytes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lookup_count_cases as LC  # noqa: E402
import riscv_mem_row_cases as M  # noqa: E402
import riscv_row_cases as A_  # noqa: E402
import rv_asm as A  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

NOT_COUNTED = ("Byte", "Range", "Program")


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


def _upload(api, canonical):
    """canonical [rows, width] (torch or numpy) -> ColMajor."""
    cm = LC.col_major(canonical)
    return api.ColMajor(api.to_device(cm), cm.shape[1], cm.shape[0])


def _count_rows(api, it, rows, prep=None):
    counter = api.LookupCounter()
    counter.add(it, _upload(api, np.array(rows, dtype=np.int64)), prep)
    return counter


def _equal_model(tables, rows):
    want_byte, want_range, _ = LC.model(rows)
    return np.array_equal(_words(tables["Byte"]), LC.monty(want_byte)) and np.array_equal(_words(tables["Range"])[0], LC.monty(want_range))


@pytest.mark.parametrize("h", LC.HEIGHTS)
def test_synthetic_shapes(api, h):
    it = LC.message_chip()
    for name, rows in LC.table_cases(h).items():
        got = _count_rows(api, it, rows).finish()
        assert (got["Byte"].height, got["Byte"].width, got["Range"].height, got["Range"].width) == (1 << 16, 6, 1 << 17, 1)
        assert _equal_model(got, rows), name
    got = _count_rows(api, it, LC.edge_rows()).finish()
    assert _equal_model(got, LC.edge_rows())


def test_every_row_on_one_cell_at_65537_rows(api):
    h = 65537
    main = torch.tensor(LC.GOOD, dtype=torch.int64).repeat(h, 1)
    counter = api.LookupCounter()
    cm = _upload(api, main)
    counter.add(LC.message_chip(), cm)
    counter.add(LC.message_chip(), cm)                         # counts add up across calls
    got = counter.finish()
    want = np.zeros(LC.RANGE_CELLS, np.int64)
    want[256 + 5] = 2 * h
    assert np.array_equal(_words(got["Range"])[0], LC.monty(want)) and not _words(got["Byte"]).any()


@pytest.mark.parametrize("name", ["one_cell", "mixed"])
def test_tables_taller_than_one_pass_of_the_grid(api, name):
    rows, want = LC.tall_tables()[name]
    assert rows.shape[0] == LC.TALL > 2048 * 256
    counter = api.LookupCounter()
    counter.add(LC.message_chip(), _upload(api, rows))
    got = counter.finish()
    assert np.array_equal(_words(got["Range"])[0], LC.monty(want)) and not _words(got["Byte"]).any()


def test_program_counters_beyond_one_pass_of_the_grid(api):
    n_instructions, pc_base = 1000, 0x200000
    pcs, want = LC.tall_program_counters(n_instructions, pc_base)
    padded = np.zeros(1024, np.int64)
    padded[:n_instructions] = want
    for events in (pcs, torch.as_tensor(np.stack([pcs] + [np.full_like(pcs, -1)] * 10, axis=1), device="cuda")):    # pcs; 11-word records
        counter = api.LookupCounter(1024)
        counter.add_program_counters(events, pc_base, n_instructions)
        got = counter.finish()
        assert np.array_equal(_words(got["Program"])[0], LC.monty(padded))
        assert not _words(got["Byte"]).any() and not _words(got["Range"]).any()


def test_a_finished_counter_takes_no_further_call(api):
    rows = LC.table_cases(65)["one_cell"]
    counter = _count_rows(api, LC.message_chip(), rows)
    got = counter.finish()
    before = _words(got["Range"]).copy()
    for call in (lambda: counter.add(LC.message_chip(), _upload(api, np.array(rows, dtype=np.int64))), counter.finish,
                 lambda: counter.add_row(LC.message_chip(), LC.monty(rows[0])),
                 lambda: counter.add_program_counters(np.array([0x200000], dtype=np.int64), 0x200000, 0)):
        with pytest.raises(RuntimeError, match="finished"):
            call()
    assert np.array_equal(_words(got["Range"]), before)
    failed = _count_rows(api, LC.message_chip(), LC.bad_table("opcode_7"))
    with pytest.raises(api._lib.Sp1HipError):
        failed.finish()
    with pytest.raises(RuntimeError, match="finished"):
        failed.finish()


def test_a_counter_on_its_own_stream(api):
    """The buffers are zeroed on the stream that counts, whatever the current stream is doing."""
    stream = torch.cuda.Stream()
    rows = LC.table_cases(257)["mixed_multiplicities"]
    table = _upload(api, np.array(rows, dtype=np.int64))
    torch.cuda.synchronize()
    counter = api.LookupCounter(stream=stream)
    counter.add(LC.message_chip(), table)
    assert _equal_model(counter.finish(), rows)


def test_weights_constants_and_preprocessed_columns(api):
    inv_rows = [(1, 8 * i + 16, 16) for i in range(65)] + [(0, 5, 1)]
    got = _count_rows(api, LC.weighted_chip(), inv_rows).finish()
    want = np.zeros(LC.RANGE_CELLS, np.int64)
    want[(1 << 13) + 1:(1 << 13) + 66] = 2
    assert np.array_equal(_words(got["Range"])[0], LC.monty(want)) and not _words(got["Byte"]).any()
    rows = LC.table_cases(65)["two_flags"]
    prep = _upload(api, np.array([r[4:6] for r in rows], dtype=np.int64))
    got = _count_rows(api, LC.message_chip(prep_columns=True), [r[:4] + (0, 0) for r in rows], prep).finish()
    assert _equal_model(got, rows)


@pytest.mark.parametrize("name", LC.SENDERS)
def test_native_device_form_equals_its_host_form(name, tmp_path):
    assert os.path.exists(LC.EXE), "tests/native/lookup_counts is not built: run __graft_entry__.build()"
    machine, tabs, _ = LC.shard()
    prep, main = tabs[name]
    args = (machine[name][1].to_array(), LC.col_major(main), LC.col_major(prep) if prep is not None else None)
    host = LC.run("host", *args, tmp_path)
    dev = LC.run("device", *args, tmp_path, timeout=60)
    for h, d, what in zip(host, dev, ("byte", "range", "status")):
        assert np.array_equal(h, d), (name, what)


@pytest.mark.parametrize("name", sorted(LC.BAD_ROWS))
def test_a_bad_message_is_an_error_and_moves_no_count(api, name):
    rows = LC.bad_table(name)
    counter = _count_rows(api, LC.message_chip(), rows)
    with pytest.raises(api._lib.Sp1HipError) as err:
        counter.finish()
    assert "send %d, row 64" % LC.SEND in str(err.value) and "Message" in str(err.value)
    assert api.to_host(counter.status)[:5].tolist() == [1, 1, LC.SEND, 64, 0]
    want_byte, want_range, bad = LC.model(rows)
    assert [r for r, _ in bad] == [64]
    counts = api.to_host(counter.counts)                        # converted in place: the good messages' counts stand
    assert np.array_equal(counts[:LC.BYTE_CELLS].reshape(6, -1), LC.monty(want_byte))
    assert np.array_equal(counts[LC.BYTE_CELLS:], LC.monty(want_range))


def test_bad_program_counters_are_errors(api):
    for pcs in ([0x200000 - 4], [0x200000 + 2], [0x200000 + 4 * 40]):
        counter = api.LookupCounter(64)
        counter.add_program_counters(np.array([0x200000, 0x200004] + pcs + [0x200004], dtype=np.int64), 0x200000, 40)
        with pytest.raises(api._lib.Sp1HipError) as err:
            counter.finish()
        assert "pc 2 of call 0" in str(err.value)
        assert api.to_host(counter.counts)[-64:-61].tolist() == LC.monty([1, 2, 0]).tolist()
    with pytest.raises(api._lib.Sp1HipError):
        api.LookupCounter().add(LC.message_chip(), api.ColMajor(api.device_words(5 * 32), 32, 5))      # a column outside the table


def _staged(api, tabs):
    return {n: (_upload(api, main), _upload(api, prep) if prep is not None else None)
            for n, (prep, main) in tabs.items() if n not in NOT_COUNTED and main.shape[0]}


def _assert_tables(got, tabs, what):
    for n in NOT_COUNTED:
        assert (got[n].height, got[n].width) == tuple(tabs[n][1].shape), (what, n)
        assert np.array_equal(_words(got[n]), LC.col_major(tabs[n][1])), (what, n)


@pytest.mark.parametrize("cases", [A_, M], ids=["alu_corner", "mem_corner"])
def test_corner_programs_equal_the_tracer(api, cases):
    ex, sh, _, _ = cases.corner()
    machine, tabs, publics = X.shard_tables(ex, sh, device="cpu")
    pc_base, program = ex.program()
    staged = _staged(api, tabs)
    _assert_tables(X.device_lookup_tables(machine, staged, publics, sh.events, program, pc_base), tabs, "staged tables, host events")
    made = X.core_device_tables(sh.events, {n: int(tabs[n][1].shape[0]) for n in tabs})
    assert made and set(made) <= set(X.ALU_TRACEGEN_CHIPS + X.MEM_TRACEGEN_CHIPS)
    swapped = {n: ((made[n], None) if n in made else t) for n, t in staged.items()}
    d_events = torch.as_tensor(sh.events, device="cuda")
    _assert_tables(X.device_lookup_tables(machine, swapped, publics, d_events, program, pc_base), tabs, "device-made tables, device events")
    packed = torch.as_tensor(np.ascontiguousarray(X.pack_alu_events(sh.events)), device="cuda")       # pc is word 0 of the records too
    _assert_tables(X.device_lookup_tables(machine, swapped, publics, packed, program, pc_base), tabs, "packed records")


def test_clock_window_tables(api):
    """The rewritten clocks are no executable history: a clock that is not 1 modulo 8 makes the 13-bit range check of
    (clk_0_16 - 1) / 8 a message that is no row of Range, in every row of these tables. So the count is an error here, and what is
    compared is everything behind it: the number of such messages, and every cell of the messages that are rows — the 16-bit checks
    of the large diff_high_limb values among them."""
    r_inv = pow(1 << 32, LC.P - 2, LC.P)
    for name, (_, table) in M.clock_window_tables().items():
        it = R.chip(name)[1]
        canonical = torch.as_tensor(((table.astype(np.uint64) * np.uint64(r_inv)) % np.uint64(LC.P)).astype(np.int64).T.copy())
        want_byte, want_range, n_bad = LC.torch_tally(it, canonical, None)
        assert want_range.sum() > 0 and n_bad > 0, name
        counter = api.LookupCounter()
        counter.add(it, api.ColMajor(api.to_device(table), table.shape[1], table.shape[0]))
        with pytest.raises(api._lib.Sp1HipError):
            counter.finish()
        assert int(api.to_host(counter.status)[0]) == n_bad, name
        counts = api.to_host(counter.counts)
        assert np.array_equal(counts[:LC.BYTE_CELLS].reshape(6, -1), LC.monty(want_byte)), name
        assert np.array_equal(counts[LC.BYTE_CELLS:], LC.monty(want_range)), name


def test_keccak_precompile_shard(api):
    from sp1_amd.machines import riscv_more_trace as MT
    machine, tabs, publics = MT.precompile_shard(1, seed=3, device="cpu")
    assert tabs["KeccakPermute"][1].shape[0] >= 24 and tabs["KeccakPermute"][1].shape[1] == 2640    # one event: 24 rows
    ctx = RT.RunContext()
    got = X.device_lookup_tables(machine, _staged(api, tabs), publics, None, ctx.program, ctx.pc_base)
    _assert_tables(got, tabs, "keccak")
    assert _words(got["Byte"]).any() and not _words(got["Program"]).any()


def test_shard_proof_with_device_counted_tables(api):
    import core_real
    p = M.all_nine_program()
    ex = X.Executor(A.elf(p.words + A.halt(0), data=M.data_bytes(), data_addr=M.DATA), stdin=[])
    sh = ex.run_shard(1 << 20)
    assert sh.halted and sh.exit_code == 0
    machine, tabs, publics = X.shard_tables(ex, sh, device="cuda")
    made = X.core_device_tables(sh.events, {n: int(tabs[n][1].shape[0]) for n in tabs})
    dev = [(a, i, core_real.to_col_major(tabs[a.name][1]), core_real.to_col_major(tabs[a.name][0]) if tabs[a.name][0] is not None else None)
           for a, i in machine]
    L, lsh, batch = 17, 12, 8
    commit, prep = api.JaggedProver(L, lsh, batch, 1).commit_multilinears([d[3] for d in dev if d[3] is not None])

    def prove(chips):
        ch = api.DuplexChallenger()
        ch.observe(commit)
        return api.prove_shard(chips, RT.to_monty_np(publics), prep, L, lsh, batch, ch, 1, 5, 4)
    want = prove(dev)
    swapped = [(a, i, made.get(a.name, m), pp) for a, i, m, pp in dev]
    assert prove(swapped) == want
    pc_base, program = ex.program()
    counted = X.device_lookup_tables(machine, {a.name: (m, pp) for a, _, m, pp in swapped if a.name not in NOT_COUNTED}, publics,
                                     torch.as_tensor(sh.events, device="cuda"), program, pc_base)
    for n in NOT_COUNTED:
        assert np.array_equal(_words(counted[n]), _words(dict((a.name, m) for a, _, m, _ in dev)[n])), n
    assert prove([(a, i, counted.get(a.name, m), pp) for a, i, m, pp in swapped]) == want
