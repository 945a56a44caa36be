"""GPU (-m gpu): device trace generation for the EdAddAssign, EdDecompress and Uint256Ops chips (sp1hip_tracegen_riscv_ed_add,
_ed_decompress, _uint256_ops), the touched words' records (sp1hip_precompile_touched_records) and device-made shards of those kinds.

* api.tracegen_riscv_ed_add / _ed_decompress / _uint256_ops at every shape of tests/ed_u256_cases.py — (0, 32) padding only, (1, 32),
  (32, 32) no padding, (33, 64) and (300, 320), across a 256-lane workgroup and, in phase B, every block index —: every word of every
  column equals the host filler's (riscv_more_trace.family_shard_from), padding rows included. The Uint256Ops events alternate their
  opcodes by row, so every wave mixes them;
* tests/native/ed_u256_rows: its device form equals its host form at (300, 320), and on two events outside the kernels'
  preconditions — ed_decompress of y = 2 and an ed_add whose 1 + d f is 0 — host against device only: Python has no expectation there;
* api.precompile_touched_records equals what family_shard_from hands _close_precompile_shard, in order;
* the argument checks;
* riscv_exec.device_family_rest_shard for every kind at 1 and 6 calls of a hand-assembled program against family_shard_from: every
  table, the public values and the Global events; for one call of each kind the proof is the same bytes from the device-made and the
  host-made tables;
* the ed25519 program and the carry program of tests/test_riscv_precompiles.py with every record of run_records built by
  device_shard_any and the host tracer's entry points patched to raise: the Global messages of all shards and the image's cancel, the
  public values chain, and the memory ends with Python's results.
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
import ed_u256_cases as C  # noqa: E402
from test_gpu_tracegen_field_chips import _assert_same_shard, _host_chips, _no_host_tables, _prep_of, _prove, _words  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more_trace as MT  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

SHARD_CALLS = (1, 6)


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _table(api, kind, ev, height):
    return getattr(api, "tracegen_riscv_" + kind)(ev, height)


# ------------------------------------------------------------------------------------------------------------ the entry points
def test_widths(api):
    lib = api._lib.load()
    for kind in C.KINDS:
        assert getattr(lib, "sp1hip_tracegen_riscv_%s_width" % kind)() == R.chip(C.CHIPS[kind])[0].main_width


@pytest.mark.parametrize("kind,n,height", C.KIND_SHAPES)
def test_every_word_equals_the_host_filler(api, kind, n, height):
    want = C.montgomery_col_major(C.host_table(kind, n, height))
    ev = torch.as_tensor(C.events(kind, n), device="cuda")
    got = _table(api, kind, ev, height)
    assert (got.width, got.height) == (want.shape[0], height)
    msg = C.first_difference(kind, want, _words(got), n)
    assert msg is None, msg


@pytest.mark.parametrize("kind", C.KINDS)
def test_argument_checks(api, kind):
    words = C.EVENT_WORDS[kind]
    ev = torch.zeros((33, words), dtype=torch.int64, device="cuda")
    with pytest.raises(api._lib.Sp1HipError):
        _table(api, kind, ev, 32)                                    # 33 rows do not fit
    with pytest.raises(api._lib.Sp1HipError):
        _table(api, kind, ev[:1], 0)
    with pytest.raises(AssertionError):
        _table(api, kind, ev[:, :words - 1].contiguous(), 64)        # not this chip's event records
    assert _table(api, kind, ev[:0], 0).words.numel() == 0


@pytest.mark.parametrize("kind", ("ed_decompress", "uint256_ops"))
@pytest.mark.parametrize("n", (1, 33, 300))
def test_the_records_are_what_the_host_filler_hands_on(api, kind, n):
    want = C.host_records(kind, n)
    got = api.precompile_touched_records(torch.as_tensor(C.events(kind, n), device="cuda"), C.FAMILY[kind]).cpu().numpy()
    assert got.shape == want.shape == (n * C.RECORDS_PER_CALL[kind], 5)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d words differ, first at record %d word %d" % (kind, len(bad), bad[0][0], bad[0][1])


def test_the_records_argument_checks(api):
    ev = torch.zeros((2, 24), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        api.precompile_touched_records(ev, 12)
    with pytest.raises(AssertionError):
        api.precompile_touched_records(ev, 14)                       # 24 words are not a uint256_ops record
    assert tuple(api.precompile_touched_records(ev[:0], 13).shape) == (0, 5)
    lib = api._lib.load()
    out = torch.zeros((16, 5), dtype=torch.int64, device="cuda")
    assert lib.sp1hip_precompile_touched_records(api._dptr(out), 15, api._dptr(ev), 2, 13, None) == api._lib.ERROR_INVALID_ARGUMENT
    assert not out.any()                                             # refused before any launch


# ---------------------------------------------------------------------------------------------------------- the native program
@pytest.mark.parametrize("kind", C.KINDS)
def test_the_native_programs_device_form_equals_its_host_form(kind, tmp_path):
    assert os.path.exists(C.EXE), "tests/native/ed_u256_rows is not built: run __graft_entry__.build()"
    n, height = C.LARGE
    ev = C.events(kind, n)
    msg = C.first_difference(kind, C.run_rows("host", kind, ev, height, tmp_path), C.run_rows("device", kind, ev, height, tmp_path), n)
    assert msg is None, msg
    if kind != "ed_add":
        assert np.array_equal(C.run_records("host", kind, ev, tmp_path), C.run_records("device", kind, ev, tmp_path))


@pytest.mark.parametrize("kind", ("ed_add", "ed_decompress"))
def test_host_and_device_agree_outside_the_preconditions(api, kind, tmp_path):
    ev = C.out_of_domain_events()[kind]
    host = C.run_rows("host", kind, ev, 32, tmp_path)
    msg = C.first_difference(kind, host, C.run_rows("device", kind, ev, 32, tmp_path), 1)
    assert msg is None, msg
    msg = C.first_difference(kind, host, _words(_table(api, kind, torch.as_tensor(ev, device="cuda"), 32)), 1)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------------------------ the shards
@pytest.fixture(scope="module")
def program_events():
    """{kind: the executor's events} of the ed25519 and carry programs run six times over: 12 ED_ADD, 12 ED_DECOMPRESS, 24 carry calls."""
    out = {}
    for program in (C.ed_program, C.carry_program):
        ex = X.Executor(program(6), stdin=[])
        for rec in X.run_records(ex, 1 << 20):
            if rec.kind in C.KINDS:
                out[rec.kind] = np.ascontiguousarray(rec.events)
    assert set(out) == set(C.KINDS)
    return out


def _both(kind, ev):
    machine, tables, publics, gev = MT.family_shard_from(kind, ev, "cpu")
    assert C.CHIPS[kind] in tables and "SyscallPrecompile" in tables
    chips = _host_chips(machine, tables)
    return (machine, chips, publics, gev), X.device_family_rest_shard(kind, ev, _prep_of(chips), RT.RunContext())


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", SHARD_CALLS)
def test_device_family_rest_shard_equals_the_host_shard(api, program_events, kind, n):
    ev = program_events[kind][:n]
    assert ev.shape == (n, C.EVENT_WORDS[kind])
    if kind == "uint256_ops" and n > 1:
        assert len(set((ev[:, 3] & 0xFF).tolist())) == 2            # both system calls in one shard
    host, device = _both(kind, ev)
    _assert_same_shard(host, device, int(host[3].shape[0]))


@pytest.mark.parametrize("kind", C.KINDS)
def test_the_proof_is_the_same_bytes_from_device_and_host_tables(api, program_events, kind):
    host, device = _both(kind, program_events[kind][:1])
    assert _prove(api, device[1], device[2]) == _prove(api, host[1], host[2])


# -------------------------------------------------------------------------------------------------------------- whole programs
@pytest.mark.parametrize("program,want", [(C.ed_program, ["core", "ed_add", "ed_decompress", "memory"]), (C.carry_program, ["core", "uint256_ops", "memory"])])
def test_a_hand_assembled_program_with_every_shard_made_on_the_device(api, program, want, monkeypatch):
    import core_real
    _no_host_tables(monkeypatch)
    ex = X.Executor(program(), stdin=[])
    prep, kinds, pvs, gevs, entry = None, [], [], [], None
    for rec in X.run_records(ex, 1 << 20):
        assert rec.kind in X.DEVICE_ANY_KINDS, rec.kind
        if prep is None:
            prep = {n: core_real.to_col_major(t) for n, t in X.preprocessed_tables(ex, "cuda").items()}
        if rec.kind == "core":
            entry = rec.executed.pc_start if entry is None else entry
        machine, chips, publics, gev9 = X.device_shard_any(ex, rec, prep)
        assert frozenset(a.name for a, _ in machine) in RT.chip_clusters() and [c[0].name for c in chips] == [a.name for a, _ in machine]
        if rec.kind in X.DEVICE_FAMILY_REST_KINDS:
            chip = X.FAMILIES[rec.kind][1]
            main = {c[0].name: c[2] for c in chips}[chip]
            assert main.height == RT.pad32(len(rec.events)) and main.width == R.chip(chip)[0].main_width
        kinds.append(rec.kind)
        pvs.append([int(v) for v in publics])
        gevs.append(X.global_events_11(gev9).cpu())
    assert kinds == want and ex.halted
    assert not X.global_events_balance(gevs + [X.image_events(ex)])
    vk_digest = X.verifying_key_words(ex, entry, "cuda")[3:]
    assert PVM.verify_proof_public_values([pvs[i] for i in X.proof_order(kinds)], entry, vk_digest) == "prev_commit_syscall doesn't equal the previous shard's commit_syscall"
    gm = {int(r[0]): int(r[2]) & C.M64 for r in ex.global_memory()}
    at = lambda off: sum(gm[C.DATA + off + 8 * k] << (64 * k) for k in range(4))
    if program is C.ed_program:
        b2, b3, x3, x_neg2 = C.ed_results()
        assert (at(0), at(32)) == b2 and (at(128), at(160)) == b3 and at(192) == x3 and at(256) == x_neg2
    else:
        for i, (code, a, b, c) in enumerate(C.CARRY_CASES):
            base = 160 * i
            full = (a * b if code & 0xFF == 0x31 else a + b) + c
            assert at(base if i == 1 else base + 96) == full & C.TOP and at(base + 128) == full >> 256
