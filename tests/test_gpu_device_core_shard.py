"""GPU: riscv_exec.device_core_shard — a provable core shard from the executor's records alone — on the three hand-assembled programs,
unshifted and shifted across 2^24 cycles (rv64_partition_cases).

* every table that has a host counterpart equals the host tracer's word for word, padding rows and height-zero chips included;
  MemoryBump is compared in the partition's canonical order (Tracer._bump_rows fed the ordered tuples) and as a multiset of rows with
  the host tracer's own table; the public values equal the host's; the returned Global events equal tr.global_events reduced to 9
  words; the preprocessed tables equal the host's;
* EventTracer.__init__ is patched to raise while device_core_shard runs: the tracer is never built;
* one shifted and one unshifted shard proved (L = 17): the bytes equal the oracle's proof from the same tables downloaded, for the
  unshifted shard also the proof from the host tracer's tables, and the pinned verifier accepts both with PVM.verifier_program();
* run_records yields the shard with the previous public values, and device_shard makes it, without a tracer being built.
Everything is bit-exact; there are no tolerances."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import pyoracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import riscv_core_row_cases as K  # noqa: E402
import riscv_row_cases as C  # noqa: E402
import rv64_partition_cases as PC  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


@functools.lru_cache(maxsize=None)
def host(which, shift):
    """(tracer after build(), machine, tables, publics) of the host path, on the CPU."""
    ex, sh = PC.shard(which, shift)
    tr = X.EventTracer(ex, sh, "cpu")
    machine, tabs, publics = tr.build()
    return tr, machine, tabs, publics


@functools.lru_cache(maxsize=None)
def prep_of(which):
    import core_real
    return {n: core_real.to_col_major(t) for n, t in X.preprocessed_tables(PC.program(which)[0], "cuda").items()}


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


def _device(which, shift, monkeypatch):
    ex, sh = PC.shard(which, shift)
    host(which, shift)                                         # the host side first: the patch below would stop it
    prep = prep_of(which)

    def refuse(self, *a, **k):
        raise AssertionError("device_core_shard built an EventTracer")
    with monkeypatch.context() as mp:
        mp.setattr(X.EventTracer, "__init__", refuse)
        return X.device_core_shard(ex, sh, prep)


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("which", PC.PROGRAMS)
def test_every_table_equals_the_host_tracers(api, which, shift, monkeypatch):
    tr, h_machine, h_tabs, h_publics = host(which, shift)
    machine, chips, publics, gev = _device(which, shift, monkeypatch)
    assert [a.name for a, _ in machine] == [a.name for a, _ in h_machine] == [c[0].name for c in chips]
    assert frozenset(a.name for a, _ in machine) in RT.chip_clusters()
    empty = 0
    for a, it, main, prep in chips:
        h_prep, h_main = h_tabs[a.name]
        assert (main.height, main.width) == tuple(h_main.shape), a.name
        empty += main.height == 0
        assert (prep is None) == (h_prep is None), a.name
        if prep is not None:
            assert np.array_equal(_words(prep), C.montgomery_col_major(h_prep)), a.name
        if main.height == 0:
            continue
        want = h_main
        if a.name == "MemoryBump":
            canonical = PC.host_tables((which, shift))[0]["MemoryBump"]
            assert sorted(map(tuple, canonical.tolist())) == sorted(map(tuple, h_main[:len(canonical)].tolist()))
            want = torch.cat([canonical, torch.zeros((main.height - len(canonical), main.width), dtype=RT.I64)])
        msg = C.first_difference(a.name, C.montgomery_col_major(want), _words(main), tr.tables[a.name].n)
        assert msg is None, msg
    assert empty >= 1 and ("MemoryBump" in tr.tables and tr.tables["MemoryBump"].n > 0) == bool(shift)
    assert torch.equal(publics, h_publics)
    assert np.array_equal(gev.cpu().numpy(), K.reduce_global_events(tr.global_events))
    assert torch.equal(X.global_events_11(gev).cpu(), tr.global_events.to(torch.int64))


def _host_arrays(chips):
    down = lambda t, w: t.to_row_major_host() if t is not None and t.height else np.zeros((0, w), np.uint32)
    return [(a, it, down(m, a.main_width), down(p, a.prep_width) if a.prep_width else None) for a, it, m, p in chips]


@pytest.mark.parametrize("shift", [False, True])
def test_the_shard_is_proved_and_verified(api, shift, monkeypatch):
    import core_real
    which = "core"
    machine, chips, publics, _ = _device(which, shift, monkeypatch)
    L, lsh, batch = 17, 12, 8
    commit, prep = api.JaggedProver(L, lsh, batch, 1).commit_multilinears([c[3] for c in chips if c[3] is not None])
    pv = RT.to_monty_np(publics)

    def prove(cs):
        ch = api.DuplexChallenger()
        ch.observe(commit)
        return api.prove_shard(cs, pv, prep, L, lsh, batch, ch, 1, 5, 4)
    got = prove(chips)
    arrays = _host_arrays(chips)
    o_prep = orc.JaggedRound([c[3] for c in arrays if c[3] is not None], L, lsh, batch, 1)
    assert np.array_equal(commit, o_prep.commit)
    o_ch = orc.Challenger()
    o_ch.observe(o_prep.commit)
    orc.set_gkr_sparse(True)
    try:
        want = orc.shard_prove(arrays, pv, o_prep, L, lsh, batch, o_ch, 1, 5, 4)
    finally:
        orc.set_gkr_sparse(False)
    assert got == want, "the proof differs from the oracle's proof of the same tables"
    if not shift:
        _, h_machine, h_tabs, h_publics = host(which, shift)
        h_chips = [(a, i, core_real.to_col_major(h_tabs[a.name][1].cuda()), core_real.to_col_major(h_tabs[a.name][0].cuda()) if h_tabs[a.name][0] is not None else None)
                   for a, i in h_machine]
        assert prove(h_chips) == got, "the proof differs from the proof of the host tracer's tables"
    v_ch = orc.Challenger()
    v_ch.observe(o_prep.commit)
    shapes = [(a, i, np.zeros((0, a.main_width), np.uint32), np.zeros((0, a.prep_width), np.uint32) if a.prep_width else None) for a, i in machine]
    assert orc.shard_verify(shapes, commit, got, L, lsh, v_ch, 1, 5, 4, pv_program=PVM.verifier_program()) == 0


def test_program_shards_yields_core_shards_untraced(api, monkeypatch):
    p = K.program()
    import rv_asm as A
    ex = X.Executor(A.elf(p.words + A.halt(0), data=K.data_bytes(), data_addr=K.DATA), stdin=[])

    def refuse(self, *a, **k):
        raise AssertionError("run_records or device_shard built an EventTracer")
    seen = []
    with monkeypatch.context() as mp:
        mp.setattr(X.EventTracer, "__init__", refuse)
        gen = X.run_records(ex, 1 << 20)
        for rec in gen:
            if rec.kind != "core":
                break
            assert rec.prev is None and rec.events is None and rec.executed is not None
            seen.append(X.device_shard(ex, rec, prep_of("core")))
            if rec.executed.halted:                            # the precompile and memory shards behind it are not this test's
                break
        gen.close()
    assert len(seen) == 1
    assert torch.equal(seen[0][2], host("core", False)[3])
