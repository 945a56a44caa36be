"""GPU (-m gpu): device-made memory and precompile shards.

* sp1hip_tracegen_riscv_memory_global through api, both kinds, on the cases and shapes of tests/memory_global_cases.py — (records,
  height) at every wave and workgroup edge the read of record i - 1 crosses —: every word of every column, padding rows included, and
  every event word equal the host tracer's (riscv_more_trace.memory_shard_from), bit for bit; the `extra_global_events` tail stays
  zero; height 0 succeeds without a launch; the argument checks through api.
* sp1hip_tracegen_riscv_syscall_precompile and sp1hip_precompile_local_records on Keccak (1, 2, 11 calls) and secp256k1 add / double
  (1, 33 calls) events against precompile_shard_from / secp256k1_*_shard_from's SyscallPrecompile and MemoryLocal tables and events.
* riscv_exec.device_memory_shard against memory_shard_from on 300 words (a first shard) and on a continuing shard with an empty Init
  list: every table and the public values are equal, and the proof is the same bytes as from the host-made tables and as the oracle's.
* riscv_exec.device_precompile_shard against the host shard at the same counts; proof bytes equal for the 2-call Keccak shard and
  for both secp256k1 shards of the hand-assembled 2G / G + 2G / 6G program.
* one run of run_records over a small fibonacci input with every shard made by device_shard: the Global events of all shards plus
  the image's cancel, and PVM.verify_proof_public_values accepts the chain."""
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import memory_global_cases as G  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more_trace as MT  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

L, LSH, BATCH = 17, 12, 8                                     # the Range table has 2^17 rows


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the entry points
@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("case,n,height", G.CASE_SHAPES)
def test_memory_global_equals_the_host_tracer(api, kind, case, n, height):
    want, want_events = G.host_table(case, kind, n, height)
    rec = torch.as_tensor(G.records3(case, kind, n), device="cuda")
    extra = 3
    got, events = api.tracegen_riscv_memory_global(kind, rec, height, G.PREVIOUS[case], extra_global_events=extra)
    assert (got.width, got.height) == (30, height)
    msg = G.first_difference(G.CHIP[kind], want, _words(got), n)
    assert msg is None, msg
    events = events.cpu().numpy()
    assert events.shape == (n + extra, 9) and events.dtype == np.int32
    assert np.array_equal(events[:n], want_events) and not events[n:].any()          # the caller's rows stay as they were


def test_memory_global_height_zero_and_argument_checks(api):
    rec = torch.zeros((33, 3), dtype=torch.int64, device="cuda")
    for kind in G.KINDS:
        table, events = api.tracegen_riscv_memory_global(kind, rec[:0], 0, 0, extra_global_events=2)
        assert table.words.numel() == 0 and tuple(events.shape) == (2, 9) and not events.cpu().numpy().any()
        with pytest.raises(api._lib.Sp1HipError):
            api.tracegen_riscv_memory_global(kind, rec, 32, 0)              # 33 rows do not fit
        with pytest.raises(api._lib.Sp1HipError):
            api.tracegen_riscv_memory_global(kind, rec[:1], 0, 0)
        with pytest.raises(AssertionError):
            api.tracegen_riscv_memory_global(kind, torch.zeros((4, 5), dtype=torch.int64, device="cuda"), 32, 0)
    with pytest.raises(KeyError):
        api.tracegen_riscv_memory_global("local", rec[:1], 32, 0)


@pytest.mark.parametrize("kind,n", [(k, n) for k in G.PRECOMPILES for n in G.PRECOMPILE_COUNTS[k]])
def test_precompile_closing_kernels_equal_the_host_builders(api, kind, n):
    import riscv_core_row_cases as K
    ev = torch.as_tensor(G.precompile_events(kind, n), device="cuda")
    _, tables, _, gev = G.host_precompile_shard(kind, n)
    words, syscall_id, arg2_word, segments = api.PRECOMPILE_DESCRIPTORS[kind]
    sp, ml = tables["SyscallPrecompile"][1], tables["MemoryLocal"][1]
    want_events = G.reduce_global_events(gev)
    records = api.precompile_local_records(ev, segments)
    n_local = int(records.shape[0])
    assert n_local == n * sum(s[1] for s in segments) and np.array_equal(records.cpu().numpy(), G.local_records_of(ml[:n_local]))
    table, events = api.tracegen_riscv_memory_local(records, int(ml.shape[0]), extra_global_events=n)
    msg = K.first_difference("MemoryLocal", G.montgomery_col_major(ml), _words(table), n_local)
    assert msg is None, msg
    assert not events[2 * n_local:].cpu().numpy().any()
    got = api.tracegen_riscv_syscall_precompile(ev, int(sp.shape[0]), syscall_id, arg2_word, global_events=events[2 * n_local:])
    msg = G.first_difference("SyscallPrecompile", G.montgomery_col_major(sp), _words(got), n)
    assert msg is None, msg
    assert np.array_equal(events.cpu().numpy(), want_events)
    alone = api.tracegen_riscv_syscall_precompile(ev, int(sp.shape[0]), syscall_id, arg2_word)          # without events
    assert np.array_equal(_words(alone), _words(got))


def test_precompile_entry_points_with_nothing_to_do_and_argument_checks(api):
    ev = torch.zeros((33, 77), dtype=torch.int64, device="cuda")
    assert api.tracegen_riscv_syscall_precompile(ev[:0], 0, 9).words.numel() == 0
    assert tuple(api.precompile_local_records(ev[:0], api.PRECOMPILE_DESCRIPTORS["keccak"][3]).shape) == (0, 5)
    with pytest.raises(api._lib.Sp1HipError):
        api.tracegen_riscv_syscall_precompile(ev, 32, 9)                    # 33 rows do not fit
    with pytest.raises(api._lib.Sp1HipError):
        api.tracegen_riscv_syscall_precompile(ev, 64, 9, arg2_word=77)      # behind the record
    with pytest.raises(api._lib.Sp1HipError):
        api.precompile_local_records(ev[:, :43].contiguous(), api.PRECOMPILE_DESCRIPTORS["keccak"][3])   # Keccak's segment in a 43-word record


# ------------------------------------------------------------------------------------------------------------------ the shards
def _host_chips(machine, tables):
    import core_real
    return [(a, i, core_real.to_col_major(tables[a.name][1].cuda()), core_real.to_col_major(tables[a.name][0].cuda()) if tables[a.name][0] is not None else None)
            for a, i in machine]


def _prep_of(chips):
    return {a.name: p for a, _, _, p in chips if p is not None}


def _assert_same_shard(host, device, n_events):
    """(machine, chips as ColMajor, publics, events [m, 11]) from the host tables against device_*_shard's return, word for word."""
    machine, chips, publics, gev = host
    d_machine, d_chips, d_publics, d_gev = device
    assert [a.name for a, _ in d_machine] == [a.name for a, _ in machine] == [c[0].name for c in d_chips]
    assert frozenset(a.name for a, _ in d_machine) in RT.chip_clusters()
    for (a, _, want, _), (_, _, got, prep) in zip(chips, d_chips):
        assert (got.width, got.height) == (want.width, want.height), a.name
        assert (prep is not None) == (a.prep_width > 0), a.name
        bad = np.argwhere(_words(want) != _words(got))
        assert not len(bad), "%s: %d words differ, first at column %d row %d" % (a.name, len(bad), bad[0][0], bad[0][1])
    assert torch.equal(d_publics, publics)
    assert d_gev.dtype == torch.int32 and tuple(d_gev.shape) == (n_events, 9)
    assert np.array_equal(d_gev.cpu().numpy(), G.reduce_global_events(gev))


def _prove(api, chips, publics):
    commit, prep = api.JaggedProver(L, LSH, BATCH, 1).commit_multilinears([c[3] for c in chips if c[3] is not None])
    ch = api.DuplexChallenger()
    ch.observe(commit)
    return api.prove_shard(chips, RT.to_monty_np(publics), prep, L, LSH, BATCH, ch, 1, 5, 4)


def _oracle_proof(machine, tables, publics):
    import pyoracle as orc
    host = [(a, i, RT.to_monty_np(tables[a.name][1]), RT.to_monty_np(tables[a.name][0]) if tables[a.name][0] is not None else None) for a, i in machine]
    prep = orc.JaggedRound([c[3] for c in host if c[3] is not None], L, LSH, BATCH, 1)
    ch = orc.Challenger()
    ch.observe(prep.commit)
    orc.set_gkr_sparse(True)                                  # the jagged-aware oracle prover (bytes equal to the dense one)
    try:
        return orc.shard_prove(host, RT.to_monty_np(publics), prep, L, LSH, BATCH, ch, 1, 5, 4)
    finally:
        orc.set_gkr_sparse(False)


@pytest.mark.parametrize("which", ["first", "continuing"])
def test_device_memory_shard_equals_the_host_shard_and_proves_to_the_same_bytes(api, which):
    if which == "first":                                      # 300 words; address 0 opens both lists
        (ia, ir), (fa, fr), previous = G.records("first", "init", 300), G.records("first", "finalize", 300), (0, 0)
    else:                                                     # nothing is initialised: MemoryGlobalInit stands at height zero, its chain still
        (ia, ir), (fa, fr), previous = G.records("continuing", "init", 0), G.records("continuing", "finalize", 65), (0x7000, G.PREVIOUS["continuing"])
    ctx = RT.RunContext()
    machine, tables, publics, gev = MT.memory_shard_from(ia, ir, fr, "cpu", previous_addr=previous[0], ctx=ctx, fin_addrs=fa, previous_fin_addr=previous[1])
    chips = _host_chips(machine, tables)
    device = X.device_memory_shard(ia, ir, fa, fr, _prep_of(chips), ctx, previous_init=previous[0], previous_fin=previous[1])
    assert [a.name for a, _ in device[0]] == sorted(RT.MEMORY_CLUSTER)
    _assert_same_shard((machine, chips, publics, gev), device, len(ia) + len(fa))
    if which == "continuing":
        assert dict((c[0].name, c[2].height) for c in device[1])["MemoryGlobalInit"] == 0
        assert PVM.get(device[2], "previous_init_addr") == PVM.get(device[2], "last_init_addr") == PVM.addr_limbs(0x7000)
    want = _prove(api, chips, publics)
    assert _prove(api, device[1], device[2]) == want
    assert want == _oracle_proof(machine, tables, publics)


@pytest.mark.parametrize("kind,n", [(k, n) for k in G.PRECOMPILES for n in G.PRECOMPILE_COUNTS[k]])
def test_device_precompile_shard_equals_the_host_shard(api, kind, n):
    machine, tables, publics, gev = G.host_precompile_shard(kind, n)
    chips = _host_chips(machine, tables)
    device = X.device_precompile_shard(kind, G.precompile_events(kind, n), _prep_of(chips), RT.RunContext())
    _assert_same_shard((machine, chips, publics, gev), device, int(gev.shape[0]))
    if (kind, n) == ("keccak", 2):
        assert _prove(api, device[1], device[2]) == _prove(api, chips, publics)


def test_both_secp256k1_shards_of_a_program_prove_to_the_same_bytes(api):
    """2G, G + 2G, 6G by the precompiles from the hand-assembled program of test_gpu_tracegen_secp.py: the two shards made on the
    device from the run's records equal the traced ones and prove to the same bytes."""
    import test_tracegen_memglobal_abi as T
    traced = {s[0]: s for s in X.program_shards(T._guest(), 1 << 20) if s[0].startswith("secp256k1_")}
    ex, seen = T._guest(), []
    for rec in X.run_records(ex, 1 << 20):
        kind = rec.kind
        if not kind.startswith("secp256k1_"):
            continue
        _, machine, tables, publics, gev, _ = traced[kind]
        chips = _host_chips(machine, tables)
        device = X.device_shard(ex, rec, _prep_of(chips))
        _assert_same_shard((machine, chips, publics, gev), device, int(gev.shape[0]))
        assert _prove(api, device[1], device[2]) == _prove(api, chips, publics)
        seen.append(kind)
    assert seen == ["secp256k1_add", "secp256k1_double"]


def test_a_whole_run_with_every_shard_made_on_the_device(api, monkeypatch):
    """fibonacci(20) with device_shard over every record of run_records: no shard has a host table and no tracer is built (the host tracer's
    entry points are patched to raise); the Global events of all shards and the image's initialisation cancel, and the public values
    chain from the entry point to HALT."""
    import core_real

    def no_tracer(*args, **kwargs):
        raise AssertionError("a host tracer was asked for a table")
    monkeypatch.setattr(X.EventTracer, "__init__", no_tracer)
    for name in ("global_chip", "byte_range_tables", "fill_cluster"):
        monkeypatch.setattr(RT.Tracer, name, no_tracer)
    for name in ("memory_shard_from", "_close_precompile_shard"):
        monkeypatch.setattr(MT, name, no_tracer)
    ex = X.Executor(X.guest_file("fibonacci.elf"), stdin=[struct.pack("<Q", 20)])
    prep, kinds, pvs, gevs, entry = None, [], [], [], None
    for rec in X.run_records(ex, 1 << 20):
        kind = rec.kind
        assert kind in X.DEVICE_KINDS, kind
        if prep is None:
            prep = {n: core_real.to_col_major(t) for n, t in X.preprocessed_tables(ex, "cuda").items()}
        if kind == "core":
            entry = rec.executed.pc_start if entry is None else entry
        machine, chips, publics, gev9 = X.device_shard(ex, rec, prep)
        assert frozenset(a.name for a, _ in machine) in RT.chip_clusters() and [c[0].name for c in chips] == [a.name for a, _ in machine]
        kinds.append(kind)
        pvs.append([int(v) for v in publics])
        gevs.append(X.global_events_11(gev9).cpu())
    assert kinds.count("core") >= 1 and kinds.count("memory") >= 1 and ex.halted
    assert not X.global_events_balance(gevs + [X.image_events(ex)])
    vk_digest = X.verifying_key_words(ex, entry, "cuda")[3:]
    assert not PVM.verify_proof_public_values([pvs[i] for i in X.proof_order(kinds)], entry, vk_digest)
