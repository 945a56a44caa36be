"""GPU (-m gpu): device trace generation for the six later instruction chips of sp1hip_tracegen_riscv_alu — Bitwise, Lt, ShiftLeft,
UType, Jal, Jalr — against the host traces of the same events (riscv_exec.shard_tables): every word of every column, padding rows
included, bit for bit, on the corner-case shard of tests/riscv_row_cases.py at (events, height) = (0, 32) padding only, (1, 32),
(32, 32) no padding, (33, 64), the whole corner set at its pad32 and (257, 288) across a 256-lane workgroup; the same with the
clocks rewritten around multiples of 2^24; the native program's device form (the library's kernels) equals its host form, which
tests/test_tracegen_riscv_host.py pins to the host tracer on the CPU; and a shard of a small hand-assembled program with rows in
all six chips proves to the same bytes from the device-generated tables as from the host tables."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import riscv_row_cases as C  # noqa: E402
import rv_asm as A  # noqa: E402

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


def _device_table(api, name, ev, height):
    got = api.tracegen_riscv_alu(name, torch.as_tensor(ev, device="cuda"), height)
    assert (got.width, got.height) == (R.chip(name)[0].main_width, height)
    return _words(got)


def test_widths(api):
    for name in C.NEW_CHIPS:
        assert api._L().sp1hip_tracegen_riscv_alu_width(api.RISCV_ALU_CHIPS[name]) == R.chip(name)[0].main_width, name
    assert api._L().sp1hip_tracegen_riscv_alu_width(14) == -1


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("name", C.NEW_CHIPS)
def test_table_equals_the_host_trace(api, name, which):
    import core_real
    n, height = C.shapes(name)[which]
    ev, want = C.case(name, n, height)
    _, _, tabs, _ = C.corner()
    if n == len(C.corner_events(name)):                        # the whole corner set: the host table as it is, through to_col_major
        assert np.array_equal(_words(core_real.to_col_major(tabs[name].cuda())), want)
    msg = C.first_difference(name, want, _device_table(api, name, ev, height), n)
    assert msg is None, msg


def test_clock_windows(api):
    for name, (ev, want) in C.clock_window_tables().items():
        msg = C.first_difference(name, want, _device_table(api, name, ev, want.shape[1]), ev.shape[0])
        assert msg is None, msg


@pytest.mark.parametrize("name", C.NEW_CHIPS)
def test_native_device_form_equals_its_host_form(name, tmp_path):
    assert os.path.exists(C.EXE), "tests/native/riscv_rows is not built: run __graft_entry__.build()"
    ev = C.corner_events(name)
    height = RT.pad32(len(ev))
    host = C.run_rows("host", name, ev, height, tmp_path)
    dev = C.run_rows("device", name, ev, height, tmp_path, timeout=60)
    msg = C.first_difference(name, host, dev, len(ev))
    assert msg is None, msg


def test_argument_checks(api):
    ev = torch.zeros((33, api.ALU_EVENT_WORDS), dtype=torch.int64, device="cuda")
    for name in C.NEW_CHIPS:
        with pytest.raises(api._lib.Sp1HipError):
            api.tracegen_riscv_alu(name, ev, 32)               # 33 rows do not fit
        with pytest.raises(api._lib.Sp1HipError):
            api.tracegen_riscv_alu(name, ev[:1], 0)
        assert api.tracegen_riscv_alu(name, ev[:0], 0).words.numel() == 0


def test_shard_proof_from_device_generated_tables(api):
    import core_real
    p = C.all_six_program()
    ex = X.Executor(A.elf(p.words + A.halt(0)), stdin=[])
    sh = ex.run_shard(1 << 20)
    assert sh.halted and sh.exit_code == 0
    machine, tabs, publics = X.shard_tables(ex, sh, device="cuda")
    ev = torch.as_tensor(sh.events, device="cuda")
    made = {}
    for name in X.ALU_TRACEGEN_CHIPS:
        main = tabs[name][1]
        if main.shape[0] == 0:
            continue
        packed = X.pack_alu_events(ev, name)
        made[name] = api.tracegen_riscv_alu(name, packed, main.shape[0])
        msg = C.first_difference(name, _words(core_real.to_col_major(main)), _words(made[name]), int(packed.shape[0]))
        assert msg is None, msg
    assert set(C.NEW_CHIPS) <= set(made)
    dev = [(a, i, core_real.to_col_major(tabs[a.name][1]), core_real.to_col_major(tabs[a.name][0]) if tabs[a.name][0] is not None else None)
           for a, i in machine]
    L, lsh, batch = 17, 12, 8
    commit, prep = api.JaggedProver(L, lsh, batch, 1).commit_multilinears([d[3] for d in dev if d[3] is not None])

    def prove(chips):
        ch = api.DuplexChallenger()
        ch.observe(commit)
        return api.prove_shard(chips, RT.to_monty_np(publics), prep, L, lsh, batch, ch, 1, 5, 4)
    want = prove(dev)
    assert prove([(a, i, made.get(a.name, m), pp) for a, i, m, pp in dev]) == want
