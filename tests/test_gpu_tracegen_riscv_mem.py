"""GPU (-m gpu): device trace generation for the nine load and store chips (sp1hip_tracegen_riscv_mem: LoadByte, LoadHalf, LoadWord,
LoadDouble, LoadX0, StoreByte, StoreHalf, StoreWord, StoreDouble) against the host traces of the same events
(riscv_exec.shard_tables): every word of every column, zero padding rows included, bit for bit, on the corner-case shard of
tests/riscv_mem_row_cases.py at (events, height) = (0, 32) padding only, (1, 32), (32, 32) no padding, (33, 64), the whole corner
set at its pad32 and (257, 288) across a 256-lane workgroup; the same with the clocks rewritten around multiples of 2^24; the native
program's device form (the library's kernels) equals its host form, which tests/test_tracegen_riscv_mem_host.py pins to the host
tracer on the CPU; the argument checks through api; and a shard of a small hand-assembled program with rows in all nine chips
proves to the same bytes from riscv_exec.core_device_tables as from the host tables."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import riscv_mem_row_cases as M  # noqa: E402
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
    got = api.tracegen_riscv_mem(name, torch.as_tensor(ev, device="cuda"), height)
    assert (got.width, got.height) == (R.chip(name)[0].main_width, height)
    return _words(got)


def test_widths(api):
    for name in M.CHIPS:
        assert api._L().sp1hip_tracegen_riscv_mem_width(api.RISCV_MEM_CHIPS[name]) == R.chip(name)[0].main_width, name
    assert api._L().sp1hip_tracegen_riscv_mem_width(9) == -1


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("name", M.CHIPS)
def test_table_equals_the_host_trace(api, name, which):
    import core_real
    n, height = M.shapes(name)[which]
    ev, want = M.case(name, n, height)
    _, _, tabs, _ = M.corner()
    if n == len(M.corner_events(name)):                        # the whole corner set: the host table as it is, through to_col_major
        assert np.array_equal(_words(core_real.to_col_major(tabs[name].cuda())), want)
    msg = M.first_difference(name, want, _device_table(api, name, ev, height), n)
    assert msg is None, msg


def test_clock_windows(api):
    for name, (ev, want) in M.clock_window_tables().items():
        msg = M.first_difference(name, want, _device_table(api, name, ev, want.shape[1]), ev.shape[0])
        assert msg is None, msg


@pytest.mark.parametrize("name", M.CHIPS)
def test_native_device_form_equals_its_host_form(name, tmp_path):
    assert os.path.exists(M.EXE), "tests/native/riscv_mem_rows is not built: run __graft_entry__.build()"
    ev = M.corner_events(name)
    height = RT.pad32(len(ev))
    host = M.run_rows("host", name, ev, height, tmp_path)
    dev = M.run_rows("device", name, ev, height, tmp_path, timeout=60)
    msg = M.first_difference(name, host, dev, len(ev))
    assert msg is None, msg


def test_argument_checks(api):
    ev = torch.zeros((33, api.MEM_EVENT_WORDS), dtype=torch.int64, device="cuda")
    for name in M.CHIPS:
        with pytest.raises(api._lib.Sp1HipError):
            api.tracegen_riscv_mem(name, ev, 32)               # 33 rows do not fit
        with pytest.raises(api._lib.Sp1HipError):
            api.tracegen_riscv_mem(name, ev[:1], 0)
        assert api.tracegen_riscv_mem(name, ev[:0], 0).words.numel() == 0
    with pytest.raises(KeyError):
        api.tracegen_riscv_mem("Add", ev, 64)                  # the other entry point's chip


def test_shard_proof_from_core_device_tables(api):
    import core_real
    p = M.all_nine_program()
    ex = X.Executor(A.elf(p.words + A.halt(0), data=M.data_bytes(), data_addr=M.DATA), stdin=[])
    sh = ex.run_shard(1 << 20)
    assert sh.halted and sh.exit_code == 0
    machine, tabs, publics = X.shard_tables(ex, sh, device="cuda")
    heights = {n: int(tabs[n][1].shape[0]) for n in tabs}
    made = X.core_device_tables(sh.events, heights)            # host events: packed on the host
    assert set(M.CHIPS) <= set(made) <= set(X.ALU_TRACEGEN_CHIPS + X.MEM_TRACEGEN_CHIPS)
    assert set(made) == {n for n in X.ALU_TRACEGEN_CHIPS + X.MEM_TRACEGEN_CHIPS if heights.get(n)}
    on_device = X.core_device_tables(torch.as_tensor(sh.events, device="cuda"), heights)        # device events: packed there
    for name, table in made.items():
        want = _words(core_real.to_col_major(tabs[name][1]))
        msg = M.first_difference(name, want, _words(table), p.rows.get(name, 0))
        assert msg is None, msg
        assert np.array_equal(_words(on_device[name]), want), name
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
