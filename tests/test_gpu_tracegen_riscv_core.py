"""GPU (-m gpu): device trace generation for DivRem, AluX0 and MemoryLocal (sp1hip_tracegen_riscv_divrem / _alu_x0 / _memory_local
through api) against the host traces of the same records, every word of every column, padding rows included, bit for bit, on the
cases of tests/riscv_core_row_cases.py — DivRem's 8 x 169 synthetic events, the hand-assembled executed program, the clocks rewritten
around multiples of 2^24, the synthetic MemoryLocal records with the Global events they send — at (records, height) = (0, 32),
(1, 32), (32, 32), (33, 64), (257, 288) and the whole set at its pad32; the argument checks through api;
riscv_exec.core_device_tables_rest on the executed program with SyscallCore's events appended: the device Global table equals the
host tracer's word for word and (global_count, digest) are the shard's public values; and the shard proved with the four
device-made tables substituted — core_device_tables' and device_lookup_tables' on top — gives the same bytes as from the host tables."""
import copy
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import riscv_core_row_cases as K  # noqa: E402
import riscv_row_cases as C  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


def _device_table(api, name, records, height, extra=0):
    """The table as uint32 [width, height] (and, for MemoryLocal, the events as int32 numpy)."""
    d = torch.as_tensor(np.ascontiguousarray(records), device="cuda")
    if name == "MemoryLocal":
        got, events = api.tracegen_riscv_memory_local(d, height, extra_global_events=extra)
    else:
        got, events = (api.tracegen_riscv_divrem if name == "DivRem" else api.tracegen_riscv_alu_x0)(d, height), None
    assert (got.width, got.height) == (R.chip(name)[0].main_width, height)
    return _words(got), None if events is None else events.cpu().numpy()


@pytest.mark.parametrize("which", range(6))
def test_divrem_synthetic_events(api, which):
    n, height = K.shapes("DivRem", "synthetic")[which]
    ev, want = K.case("DivRem", n, height, "synthetic")
    msg = K.first_difference("DivRem", want, _device_table(api, "DivRem", ev, height)[0], n)
    assert msg is None, msg


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("name", K.CHIPS)
def test_executed_program_equals_the_host_tracer(api, name, which):
    n, height = K.shapes(name)[which]
    ev, want = K.case(name, n, height)
    got, events = _device_table(api, name, ev, height)
    msg = K.first_difference(name, want, got, n)
    assert msg is None, msg
    if name == "MemoryLocal":
        assert np.array_equal(events, K.memory_local_host(ev)[1] if n else np.zeros((0, 9), np.int32))


def test_clock_windows(api):
    for name, (ev, want) in K.clock_window_tables().items():
        msg = K.first_difference(name, want, _device_table(api, name, ev, want.shape[1])[0], ev.shape[0])
        assert msg is None, msg


def test_memory_local_synthetic_records_and_their_global_events(api):
    records = K.synthetic_records()
    table, events = K.memory_local_host(records)
    n, height, extra = len(records), table.shape[0], 3
    got, got_events = _device_table(api, "MemoryLocal", records, height, extra=extra)
    msg = K.first_difference("MemoryLocal", C.montgomery_col_major(table), got, n)
    assert msg is None, msg
    assert got_events.shape == (2 * n + extra, 9) and got_events.dtype == np.int32
    assert np.array_equal(got_events[:2 * n], events) and not got_events[2 * n:].any()          # the caller's rows stay as they were


def test_argument_checks(api):
    ev = torch.zeros((33, api.ALU_EVENT_WORDS), dtype=torch.int64, device="cuda")
    for fn in (api.tracegen_riscv_divrem, api.tracegen_riscv_alu_x0):
        with pytest.raises(api._lib.Sp1HipError):
            fn(ev, 32)                                         # 33 rows do not fit
        with pytest.raises(api._lib.Sp1HipError):
            fn(ev[:1], 0)
        assert fn(ev[:0], 0).words.numel() == 0
    rec = torch.zeros((33, api.MEMORY_LOCAL_RECORD_WORDS), dtype=torch.int64, device="cuda")
    with pytest.raises(api._lib.Sp1HipError):
        api.tracegen_riscv_memory_local(rec, 32)
    table, events = api.tracegen_riscv_memory_local(rec[:0], 0, extra_global_events=2)
    assert table.words.numel() == 0 and tuple(events.shape) == (2, 9)


def _syscall_global_events(tr):
    t = tr.tables["SyscallCore"]
    return torch.cat([v for _, v, _ in RT.eval_interactions(R.chip("SyscallCore")[1], t.main[:t.n], None, kinds=(R.GLOBAL,))])


def test_core_device_tables_rest_makes_the_global_table(api):
    import core_real
    _, sh, tr, tabs, rows = K.executed()
    syscalls = _syscall_global_events(tr)
    assert syscalls.shape[0] >= 1 and syscalls.shape[1] == 11
    heights = {n: int(t.shape[0]) for n, t in tabs.items()}
    on_device = copy.copy(sh)
    on_device.events = torch.as_tensor(sh.events, device="cuda")
    for shard in (sh, on_device):                              # host events, then device events: packed where they are
        made, (count, digest) = X.core_device_tables_rest(shard, heights, syscall_global_events=syscalls)
        assert set(made) == set(X.REST_TRACEGEN_CHIPS)
        for name, table in made.items():
            want = _words(core_real.to_col_major(tabs[name].cuda()))
            msg = K.first_difference(name, want, _words(table), count if name == "Global" else len(sh.local) if name == "MemoryLocal" else rows[name])
            assert msg is None, msg
        assert heights["Global"] > count == 2 * len(sh.local) + syscalls.shape[0] == tr.global_events.shape[0]      # padding rows were compared
        publics = PVM.to_tensor(tr.pv)
        assert count == PVM.get(publics, "global_count") and digest == PVM.get(publics, "global_cumulative_sum") and len(digest) == 14
    none, (count, _) = X.core_device_tables_rest(sh, {"AluX0": heights["AluX0"]})
    assert set(none) == {"AluX0"} and count == 2 * len(sh.local)


def test_shard_proof_from_the_device_made_tables(api):
    import core_real
    ex, sh, tr, _, _ = K.executed()
    machine, tabs, publics = X.shard_tables(ex, sh, device="cuda")
    heights = {n: int(tabs[n][1].shape[0]) for n in tabs}
    dev = [(a, i, core_real.to_col_major(tabs[a.name][1]), core_real.to_col_major(tabs[a.name][0]) if tabs[a.name][0] is not None else None)
           for a, i in machine]
    L, lsh, batch = 17, 12, 8
    commit, prep = api.JaggedProver(L, lsh, batch, 1).commit_multilinears([d[3] for d in dev if d[3] is not None])

    def prove(chips):
        ch = api.DuplexChallenger()
        ch.observe(commit)
        return api.prove_shard(chips, RT.to_monty_np(publics), prep, L, lsh, batch, ch, 1, 5, 4)
    want = prove(dev)
    rest, _ = X.core_device_tables_rest(sh, heights, syscall_global_events=_syscall_global_events(tr))
    assert set(rest) == set(X.REST_TRACEGEN_CHIPS)
    swapped = [(a, i, rest.get(a.name, m), pp) for a, i, m, pp in dev]
    assert prove(swapped) == want
    core = X.core_device_tables(sh.events, heights)
    assert core and not set(core) & set(rest)
    swapped = [(a, i, core.get(a.name, m), pp) for a, i, m, pp in swapped]
    pc_base, program = ex.program()
    skip = ("Byte", "Range", "Program")
    counted = X.device_lookup_tables(machine, {a.name: (m, pp) for a, _, m, pp in swapped if a.name not in skip}, publics,
                                     torch.as_tensor(sh.events, device="cuda"), program, pc_base)
    assert prove([(a, i, counted.get(a.name, m), pp) for a, i, m, pp in swapped]) == want
