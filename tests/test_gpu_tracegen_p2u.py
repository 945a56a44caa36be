"""GPU (-m gpu): device trace generation for the Poseidon2 and Uint256MulMod chips and device-made POSEIDON2 / UINT256_MUL shards.

* the two entry points through api at every shape of tests/p2u_cases.py — (events, height) on the wave and workgroup edges —: every
  word of every column equals the host builder's (riscv_more_trace.poseidon2_shard_from / uint256_shard_from), padding rows included;
  height 0 gives an empty table; too many events for the height and a record of the wrong width raise;
* tests/native/p2u_rows: its device form equals its host form, for the rows and for the division alone — every surviving triple of
  the operand set and the two outside the chip's domain (ordinary wrapped arithmetic with a fixed trip count);
* riscv_exec.device_precompile_shard for both kinds at 1 and 6 calls against the host shard: every table, the public values and the
  Global events; for one call of each kind the proof is the same bytes from the device-made and the host-made tables;
* the two hand-assembled programs of tests/test_riscv_exec.py with every record of run_records built by device_shard and the host
  tracer's entry points patched to raise: the Global events of all shards and the image's cancel, and the memory ends with Python's
  results;
* the poseidon2 guest (input 20, 2^20 cycles per shard) the same way: core, poseidon2, sha_extend, sha_compress, memory, all
  device-made; the messages cancel and PVM.verify_proof_public_values accepts the chain.
Everything is bit-exact; there are no tolerances."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import memory_global_cases as G  # noqa: E402
import p2u_cases as C  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more_trace as MT  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

L, LSH, BATCH = 17, 12, 8                                     # the Range table has 2^17 rows
WRAPPER = {"poseidon2": "tracegen_riscv_poseidon2", "uint256": "tracegen_riscv_uint256_mul"}


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------ the entry points
def test_widths(api):
    lib = api._lib.load()
    assert lib.sp1hip_tracegen_riscv_poseidon2_width() == R.chip("Poseidon2")[0].main_width == 348
    assert lib.sp1hip_tracegen_riscv_uint256_mul_width() == R.chip("Uint256MulMod")[0].main_width == 371


@pytest.mark.parametrize("kind,n,height", C.KIND_SHAPES)
def test_every_word_equals_the_host_builder(api, kind, n, height):
    want = C.montgomery_col_major(C.host_table(kind, n, height))
    ev = torch.as_tensor(C.events(kind, n), device="cuda")
    got = getattr(api, WRAPPER[kind])(ev, height)
    assert (got.width, got.height) == (want.shape[0], height)
    msg = C.first_difference(kind, want, _words(got), n)
    assert msg is None, msg
    if n:
        assert np.array_equal(_words(api.tracegen_riscv_records(C.CHIPS[kind], ev, height)), _words(got))


@pytest.mark.parametrize("kind", C.KINDS)
def test_argument_checks(api, kind):
    fn, words = getattr(api, WRAPPER[kind]), C.WORDS[kind]
    ev = torch.zeros((33, words), dtype=torch.int64, device="cuda")
    with pytest.raises(api._lib.Sp1HipError):
        fn(ev, 32)                                               # 33 rows do not fit
    with pytest.raises(api._lib.Sp1HipError):
        fn(ev[:1], 0)
    with pytest.raises(AssertionError):
        fn(ev[:, :words - 1].contiguous(), 64)                   # not this chip's event records
    assert fn(ev[:0], 0).words.numel() == 0


# ---------------------------------------------------------------------------------------------------------- the native program
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n,height", [(0, 32), (65, 96), (300, 320)])
def test_the_native_programs_device_form_equals_its_host_form(kind, n, height, tmp_path):
    ev = C.events(kind, n)
    msg = C.first_difference(kind, C.run_rows("host", kind, ev, height, tmp_path), C.run_rows("device", kind, ev, height, tmp_path), n)
    assert msg is None, msg


def test_the_division_on_the_device_equals_the_host_form_and_divmod(tmp_path):
    triples = C.TRIPLES + C.OUTSIDE
    got = C.run_div("device", triples, tmp_path)
    assert got == C.run_div("host", triples, tmp_path)
    for (x, y, m), (result, carry) in zip(triples, got):
        q, r = divmod(x * y, C.modulus_of(m))
        assert (result, carry) == (r, q % C.B256), (hex(x), hex(y), hex(m))


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


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", C.SHARD_CALLS)
def test_device_precompile_shard_equals_the_host_shard(api, kind, n):
    ev = C.shard_events(kind, n)
    machine, tables, publics, gev = C.host_shard(kind, n)
    assert C.CHIPS[kind] in tables
    chips = _host_chips(machine, tables)
    device = X.device_precompile_shard(kind, ev, _prep_of(chips), RT.RunContext())
    _assert_same_shard((machine, chips, publics, gev), device, int(gev.shape[0]))
    if n == 1:
        assert _prove(api, device[1], device[2]) == _prove(api, chips, publics)


# -------------------------------------------------------------------------------------------------------------- whole programs
def _no_host_tables(monkeypatch):
    def no_tracer(*args, **kwargs):
        raise AssertionError("a host tracer was asked for a table")
    monkeypatch.setattr(X.EventTracer, "__init__", no_tracer)
    for name in ("global_chip", "byte_range_tables", "fill_cluster"):
        monkeypatch.setattr(RT.Tracer, name, no_tracer)
    for name in ("memory_shard_from", "_close_precompile_shard", "sha_extend_shard_from", "sha_compress_shard_from", "poseidon2_shard_from", "uint256_shard_from"):
        monkeypatch.setattr(MT, name, no_tracer)


def _device_run(ex, max_cycles, want_chips):
    """Every record of the run through device_shard: (kinds, public values, Global events [m, 11] per shard, entry pc)."""
    import core_real
    prep, kinds, pvs, gevs, entry = None, [], [], [], None
    for rec in X.run_records(ex, max_cycles):
        kind = rec.kind
        assert kind in X.DEVICE_SHARD_KINDS, kind
        if prep is None:
            prep = {n: core_real.to_col_major(t) for n, t in X.preprocessed_tables(ex, "cuda").items()}
        if kind == "core":
            entry = rec.executed.pc_start if entry is None else entry
        machine, chips, publics, gev9 = X.device_shard(ex, rec, prep)
        assert frozenset(a.name for a, _ in machine) in RT.chip_clusters() and [c[0].name for c in chips] == [a.name for a, _ in machine]
        if kind in want_chips:
            main = {c[0].name: c[2] for c in chips}[want_chips[kind]]
            assert main.height == RT.pad32(len(rec.events)) and main.width == R.chip(want_chips[kind])[0].main_width
        kinds.append(kind)
        pvs.append([int(v) for v in publics])
        gevs.append(X.global_events_11(gev9).cpu())
    return kinds, pvs, gevs, entry


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_hand_assembled_program_with_every_shard_made_on_the_device(api, kind, monkeypatch):
    _no_host_tables(monkeypatch)
    program, memory, _ = C.PROGRAMS[kind]
    ex = X.Executor(program(), stdin=[])
    kinds, _, gevs, _ = _device_run(ex, 1 << 20, {kind: C.CHIPS[kind]})
    assert kinds == ["core", kind, "memory"] and ex.halted
    assert not X.global_events_balance(gevs + [X.image_events(ex)])
    gm = {int(r[0]): int(r[2]) & C.M64 for r in ex.global_memory()}
    for addr, word in memory().items():
        assert gm[addr] == word, hex(addr)


def test_the_poseidon2_guest_with_every_shard_made_on_the_device(api, monkeypatch):
    """poseidon2.elf on input 20, 2^20 cycles per shard, with device_shard over every record of run_records: no shard has a host table
    and no tracer is built; the Global events of all shards and the image's initialisation cancel, and the public values chain from
    the entry point to HALT."""
    import test_tracegen_memglobal_abi as T
    _no_host_tables(monkeypatch)
    guest, max_cycles = T.RUNS["poseidon2"]
    ex = guest()
    kinds, pvs, gevs, entry = _device_run(ex, max_cycles, {"poseidon2": "Poseidon2"})
    assert kinds == ["core", "poseidon2", "sha_extend", "sha_compress", "memory"] and ex.halted
    assert not X.global_events_balance(gevs + [X.image_events(ex)])
    vk_digest = X.verifying_key_words(ex, entry, "cuda")[3:]
    assert not PVM.verify_proof_public_values([pvs[i] for i in X.proof_order(kinds)], entry, vk_digest)
