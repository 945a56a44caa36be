"""GPU: api.partition_rv64_events (sp1hip_rv64_partition_count / _scatter) against a numpy stable partition, and the four small
chips' kernels through sp1_amd.api against the host fillers.

* the partition: every bin's records equal and in order, the counts equal, two calls identical bytes — at n = 0, 1, 63, 64, 65, one
  workgroup's events - 1, +- 0, + 1, SCAN_SLICES workgroups + 0, + 1 workgroup (the scan's slices then hold two workgroups each), + 1
  event, and 3 SCAN_SLICES + 1 workgroups (four to a slice, the last slice partial, most slices unused) — sizes from the header's
  constants — on five streams tiled from the three hand-assembled programs' events, shifted and unshifted, and the synthetic events:
  every bin non-empty (the events interleaved so that every prefix of a workgroup or more holds all 29 bins — asserted on the
  events sent — and the whole stream once), all events in one bin, every event adding three MemoryBump records, a wave's 64 events
  in 26 different bins, and StateBump / SyscallCore records several to a wave and in every wave of a workgroup;
* SyscallInstrs, SyscallCore (with its Global events), StateBump and MemoryBump: the CPU cases of test_tracegen_riscv_sys_host.py,
  word for word, padding included.
Everything is bit-exact; there are no tolerances."""
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import riscv_row_cases as C  # noqa: E402
import rv64_partition_cases as PC  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _constant(name):
    return int(re.search(r"#define %s (\d+)" % name, open(os.path.join(ROOT, "include", "sp1hip.h")).read()).group(1))


WG, SLICES = _constant("SP1HIP_RV64_PARTITION_WORKGROUP"), _constant("SP1HIP_RV64_PARTITION_SCAN_SLICES")
SIZES = [0, 1, 63, 64, 65, WG - 1, WG, WG + 1, SLICES * WG, (SLICES + 1) * WG, (SLICES + 1) * WG + 1, (3 * SLICES + 1) * WG]


def _interleaved(ev):
    """The events reordered so that the k-th event of every kind — chip, and whether it adds a SyscallCore, a StateBump, MemoryBump
    records — comes before the (k + 1)-th of any: every prefix longer than the number of kinds holds every kind that occurs."""
    sc, sb, _, _, bumps = PC.conditions(ev)
    kind = ["%s %d %d %d" % t for t in zip(X.chip_of_events(ev), sc, sb, bumps.any(axis=1))]
    seen, nth = {}, np.zeros(len(ev), dtype=np.int64)
    for i, k in enumerate(kind):
        nth[i] = seen[k] = seen.get(k, -1) + 1
    assert len(seen) < WG - 1
    return ev[np.argsort(nth, kind="stable")]


def _streams():
    every = _interleaved(np.concatenate([PC.source_events(s)[2] for s in PC.SOURCES]))
    alu = PC.program("alu")[1].events
    one_bin = alu[X.chip_of_events(alu) == "Add"]
    three = PC.synthetic_bump_events()
    three = three[PC.conditions(three)[4].all(axis=1)]
    names = X.chip_of_events(every)
    firsts = [every[np.nonzero(names == n)[0][0]] for n in PC.BINS[:26]]
    mixed = np.array([firsts[i % 26] for i in range(64)], dtype=np.int64)
    both = [PC.synthetic_state_events(), PC.synthetic_ecalls()]                # alternating, so that every wave holds both kinds
    order = np.argsort(np.concatenate([2 * np.arange(len(b)) + k for k, b in enumerate(both)]), kind="stable")
    state = np.concatenate(both)[order]
    return {"every": every, "one_bin": one_bin, "three_bumps": three, "mixed_wave": mixed, "state_and_syscalls": state}


@pytest.mark.parametrize("stream", ["every", "one_bin", "three_bumps", "mixed_wave", "state_and_syscalls"])
def test_partition_equals_the_numpy_stable_partition(api, stream):
    base = _streams()[stream]
    assert len(base)
    sizes = SIZES + [len(base)] if stream == "every" else SIZES
    if stream == "state_and_syscalls":                          # several of each in every wave of a tiled workgroup
        sc, sb = PC.conditions(C.take(base, WG))[:2]
        assert all(sb[w:w + 64].sum() >= 4 and sc[w:w + 64].sum() >= 2 for w in range(0, WG, 64))
    elif stream == "every":
        assert len(base) > (SLICES + 1) * WG + 1
    elif stream == "one_bin":
        assert [n for n, v in PC.reference_partition(base).items() if len(v)] == ["Add"]
    elif stream == "three_bumps":
        assert len(PC.reference_partition(base)["MemoryBump"]) == 3 * len(base)
    else:
        assert len(set(X.chip_of_events(base[:64]))) == 26
    for n in sizes:
        ev = np.ascontiguousarray(C.take(base, n)).reshape(-1, X.EV_WORDS)
        want = PC.reference_partition(ev)
        if stream == "every" and n >= WG - 1:
            assert all(len(v) for v in want.values()), (n, [k for k, v in want.items() if not len(v)])
        d_ev = torch.as_tensor(ev, device="cuda")
        got, again = api.partition_rv64_events(d_ev), api.partition_rv64_events(d_ev)
        assert tuple(got) == PC.BINS
        for name, w in zip(PC.BINS, PC.BIN_WORDS):
            g = got[name].cpu().numpy()
            assert g.shape == want[name].shape == (len(want[name]), w), (stream, n, name, g.shape, want[name].shape)
            assert np.array_equal(g, want[name]), (stream, n, name, np.argwhere(g != want[name])[:4])
            assert torch.equal(got[name], again[name]), (stream, n, name)


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", PC.SYS_CHIPS)
def test_the_four_chips_equal_the_host_fillers(api, name):
    gen = {"SyscallInstrs": api.tracegen_riscv_syscall_instrs, "SyscallCore": api.tracegen_riscv_syscall_core,
           "StateBump": api.tracegen_riscv_state_bump, "MemoryBump": api.tracegen_riscv_memory_bump}[name]
    words = PC.BIN_WORDS[PC.BINS.index(name)]
    rows = 0
    for source in PC.SOURCES:
        for n, height in PC.shapes(source, name):
            rec, want = PC.case(source, name, n, height)
            got = gen(torch.as_tensor(rec.reshape(-1, words), device="cuda"), height)
            assert (got.width, got.height) == (R.chip(name)[0].main_width, height)
            msg = C.first_difference(name, want, _words(got), n)
            assert msg is None, (source, msg)
            rows += n
    assert rows > 257


def test_syscall_core_writes_its_global_events_behind_memory_locals(api):
    for source in (("core", False), ("ecalls", None)):
        _, records, events = PC.host_tables(source)
        rec = torch.as_tensor(records["SyscallCore"], device="cuda")
        m = len(events)
        assert m > 0
        local = torch.as_tensor(PC.program("core")[1].local[:5], device="cuda").contiguous()
        _, gev = api.tracegen_riscv_memory_local(local, 32, extra_global_events=m)
        before = gev[:10].clone()
        api.tracegen_riscv_syscall_core(rec, 32 * (-(-m // 32)), global_events=gev[10:])
        assert torch.equal(gev[:10], before)
        assert np.array_equal(gev[10:].cpu().numpy(), events)
