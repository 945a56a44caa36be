"""GPU (-m gpu): device trace generation for the SHA-256 precompile chips and device-made SHA_EXTEND / SHA_COMPRESS shards.

* the four entry points through api at every shape of tests/sha_cases.py — (calls, height) across the 64-lane and 256-lane edges —:
  every word of every column equals the host builder's (riscv_more_trace.sha_extend_shard_from / sha_compress_shard_from), padding
  rows included, and the restated padding behind the host builder's own height; height 0 gives an empty table; too many events for
  the height and a record of the wrong width raise;
* api.precompile_local_records with both SHA descriptors against the host shard's MemoryLocal records; a quad segment that reads
  behind the record raises;
* riscv_exec.device_precompile_shard for both kinds at 1 and 6 calls against the host shard: every table, the public values and the
  Global events; for one call of each kind the proof is the same bytes from the device-made and the host-made tables and the oracle's;
* the sha2 guest with every record of run_records built by device_shard and the host tracer's entry points patched to raise: the
  kinds are core, core, sha_extend, sha_compress, memory, the Global events of all shards and the image's cancel, and
  PVM.verify_proof_public_values accepts the chain.
Everything is bit-exact; there are no tolerances."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import memory_global_cases as G  # noqa: E402
import sha_cases as S  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more_trace as MT  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

L, LSH, BATCH = 17, 12, 8                                     # the Range table has 2^17 rows
WRAPPER = {"ShaExtend": "tracegen_riscv_sha_extend", "ShaExtendControl": "tracegen_riscv_sha_extend_control",
           "ShaCompress": "tracegen_riscv_sha_compress", "ShaCompressControl": "tracegen_riscv_sha_compress_control"}


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the entry points
@pytest.mark.parametrize("chip,n,height", S.CHIP_SHAPES)
def test_every_word_equals_the_host_builder(api, chip, n, height):
    want = S.montgomery_col_major(S.expected_table(chip, n, height))
    ev = torch.as_tensor(S.events(S.KIND_OF[chip], n), device="cuda")
    got = getattr(api, WRAPPER[chip])(ev, height)
    assert (got.width, got.height) == (want.shape[0], height)
    msg = S.first_difference(chip, want, _words(got), S.ROWS_PER_CALL[chip] * n)
    assert msg is None, msg
    if n:
        assert np.array_equal(_words(api.tracegen_riscv_records(chip, ev, height)), _words(got))


@pytest.mark.parametrize("chip", sorted(WRAPPER))
def test_height_zero_and_argument_checks(api, chip):
    kind, rows = S.KIND_OF[chip], S.ROWS_PER_CALL[chip]
    ev = torch.as_tensor(S.events(kind, 33), device="cuda")
    run = getattr(api, WRAPPER[chip])
    assert run(ev[:0], 0).words.numel() == 0
    with pytest.raises(api._lib.Sp1HipError):
        run(ev, 33 * rows - 1)                                # the last call's rows do not fit
    with pytest.raises(api._lib.Sp1HipError):
        run(ev[:1], 0)
    with pytest.raises(AssertionError):
        run(ev[:, :-1].contiguous(), 64 * rows)               # a record of the wrong width
    with pytest.raises(AssertionError):
        run(torch.as_tensor(S.events(S.KINDS[1 - S.KINDS.index(kind)], 1), device="cuda"), 96)      # the other kind's record


# ----------------------------------------------------------------------------------------------------------- the local records
@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("n", S.SHARD_CALLS)
def test_local_records_equal_the_host_shards(api, kind, n):
    ev = S.shard_events(kind, n)
    _, tables, _, _ = S.host_shard(kind, ev, key=(kind, n))
    words, _, _, segments = api.SHA_DESCRIPTORS[kind]
    assert words == ev.shape[1] and segments == S.SEGMENTS[kind]
    records = api.precompile_local_records(torch.as_tensor(ev, device="cuda"), segments)
    per_call = sum(s[1] for s in segments)
    assert tuple(records.shape) == (per_call * n, 5)
    assert np.array_equal(records.cpu().numpy(), G.local_records_of(tables["MemoryLocal"][1][:per_call * n]))


def test_a_quad_segment_that_reads_behind_the_record_raises(api):
    ev = torch.as_tensor(S.events("sha_extend", 1), device="cuda")
    quad = api.PRECOMPILE_QUAD_WORDS
    assert tuple(api.precompile_local_records(ev, ((1, 64, 530, quad, 0),)).shape) == (64, 5)
    assert tuple(api.precompile_local_records(ev[:0], ((1, 64, 530, quad, 0),)).shape) == (0, 5)
    for bad in ((1, 64, 531, quad, 0), (1, 65, 530, quad, 0), (1, 197, 0, quad, 0)):
        with pytest.raises(api._lib.Sp1HipError):
            api.precompile_local_records(ev, (bad,))
    with pytest.raises(api._lib.Sp1HipError):                 # SHA_EXTEND's segment in a 155-word record
        api.precompile_local_records(torch.as_tensor(S.events("sha_compress", 1), device="cuda"), api.SHA_DESCRIPTORS["sha_extend"][3])


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


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("n", S.SHARD_CALLS)
def test_device_precompile_shard_equals_the_host_shard(api, kind, n):
    ev = S.shard_events(kind, n)
    machine, tables, publics, gev = S.host_shard(kind, ev, key=(kind, n))
    assert set(S.CHIPS[kind]) <= set(tables)
    chips = _host_chips(machine, tables)
    device = X.device_precompile_shard(kind, ev, _prep_of(chips), RT.RunContext())
    _assert_same_shard((machine, chips, publics, gev), device, int(gev.shape[0]))
    if n == 1:
        want = _prove(api, chips, publics)
        assert _prove(api, device[1], device[2]) == want
        assert want == _oracle_proof(machine, tables, publics)


def test_the_sha2_guest_with_every_shard_made_on_the_device(api, monkeypatch):
    """sha2.elf on bytes(range(200)), 8000 cycles per shard, with device_shard over every record of run_records: no shard has a host
    table and no tracer is built (the host tracer's entry points are patched to raise); the Global events of all shards and the
    image's initialisation cancel, and the public values chain from the entry point to HALT."""
    import core_real
    import test_tracegen_memglobal_abi as T

    def no_tracer(*args, **kwargs):
        raise AssertionError("a host tracer was asked for a table")
    monkeypatch.setattr(X.EventTracer, "__init__", no_tracer)
    for name in ("global_chip", "byte_range_tables", "fill_cluster"):
        monkeypatch.setattr(RT.Tracer, name, no_tracer)
    for name in ("memory_shard_from", "_close_precompile_shard", "sha_extend_shard_from", "sha_compress_shard_from"):
        monkeypatch.setattr(MT, name, no_tracer)
    guest, max_cycles = T.RUNS["sha2"]
    ex = guest()
    prep, kinds, pvs, gevs, entry = None, [], [], [], None
    for rec in X.run_records(ex, max_cycles):
        kind = rec.kind
        assert kind in X.DEVICE_KINDS, kind
        if prep is None:
            prep = {n: core_real.to_col_major(t) for n, t in X.preprocessed_tables(ex, "cuda").items()}
        if kind == "core":
            entry = rec.executed.pc_start if entry is None else entry
        machine, chips, publics, gev9 = X.device_shard(ex, rec, prep)
        assert frozenset(a.name for a, _ in machine) in RT.chip_clusters() and [c[0].name for c in chips] == [a.name for a, _ in machine]
        if kind in S.KINDS:
            assert set(S.CHIPS[kind]) <= set(a.name for a, _ in machine)
        kinds.append(kind)
        pvs.append([int(v) for v in publics])
        gevs.append(X.global_events_11(gev9).cpu())
    assert kinds == ["core", "core", "sha_extend", "sha_compress", "memory"] and ex.halted
    assert not X.global_events_balance(gevs + [X.image_events(ex)])
    vk_digest = X.verifying_key_words(ex, entry, "cuda")[3:]
    assert not PVM.verify_proof_public_values([pvs[i] for i in X.proof_order(kinds)], entry, vk_digest)
