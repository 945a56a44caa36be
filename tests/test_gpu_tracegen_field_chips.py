"""GPU (-m gpu): device trace generation for the twelve Weierstrass and Fp / Fp2 precompile chips (sp1hip_tracegen_riscv_field_chip,
SP1HIP_RV64_FAMILY_* 0..11) and device-made shards of those kinds.

* api.tracegen_riscv_field_chip at every shape of tests/field_chip_cases.py — (0, 32) padding only, (1, 32), (32, 32) no padding,
  (33, 64) for all twelve kinds and (300, 320), across a 256-lane workgroup and, in phase B, every operation index, for one N = 8
  and one N = 12 kind of each shape —: every word of every column equals the host filler's (riscv_more_trace.family_shard_from),
  padding rows included. The Fp and Fp2 add / sub events cycle their opcodes by row, so every wave mixes them;
* tests/native/field_chip_rows: its device form equals its host form;
* the argument checks, families 12..14 among them;
* riscv_exec.device_family_shard for every kind at 1 and 6 calls of a hand-assembled program against family_shard_from: every
  table, the public values and the Global events; for bn254_add, bls12381_double, bn254_fp (three opcodes in one shard) and
  bls12381_fp2_mul the proof is the same bytes from the device-made and the host-made tables;
* the hand-assembled programs of tests/test_riscv_precompiles.py for one curve (secp256r1: a != 0) and one tower field (bls12-381)
  with every record of run_records built by device_shard_of and the host tracer's entry points patched to raise: the Global
  messages of all shards and the image's cancel, the public values chain, and the memory ends with Python's results.
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
import field_chip_cases as C  # noqa: E402
import memory_global_cases as G  # noqa: E402

from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more as M  # noqa: E402
from sp1_amd.machines import riscv_more_trace as MT  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

L, LSH, BATCH = 17, 12, 8                                     # the Range table has 2^17 rows
SHARD_CALLS = (1, 6)
PROOFS = [("bn254_add", 1), ("bls12381_double", 2), ("bn254_fp", 3), ("bls12381_fp2_mul", 1)]


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _words(col_major):
    return col_major.words.view(col_major.width, col_major.height).cpu().numpy().view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- the entry point
def test_widths(api):
    lib = api._lib.load()
    for kind in C.KINDS:
        assert lib.sp1hip_tracegen_riscv_field_chip_width(C.FAMILY[kind]) == R.chip(C.CHIPS[kind])[0].main_width
    assert [lib.sp1hip_tracegen_riscv_field_chip_width(f) for f in (12, 13, 14, 15)] == [-1] * 4


@pytest.mark.parametrize("kind,n,height", C.KIND_SHAPES)
def test_every_word_equals_the_host_filler(api, kind, n, height):
    want = C.montgomery_col_major(C.host_table(kind, n, height))
    ev = torch.as_tensor(C.events(kind, n), device="cuda")
    got = api.tracegen_riscv_field_chip(kind, ev, height)
    assert (got.width, got.height) == (want.shape[0], height)
    msg = C.first_difference(kind, want, _words(got), n)
    assert msg is None, msg


@pytest.mark.parametrize("kind", C.KINDS)
def test_argument_checks(api, kind):
    words = C.event_words(kind)
    ev = torch.zeros((33, words), dtype=torch.int64, device="cuda")
    with pytest.raises(api._lib.Sp1HipError):
        api.tracegen_riscv_field_chip(kind, ev, 32)                  # 33 rows do not fit
    with pytest.raises(api._lib.Sp1HipError):
        api.tracegen_riscv_field_chip(kind, ev[:1], 0)
    with pytest.raises(AssertionError):
        api.tracegen_riscv_field_chip(kind, ev[:, :words - 1].contiguous(), 64)      # not this chip's event records
    assert api.tracegen_riscv_field_chip(kind, ev[:0], 0).words.numel() == 0


def test_the_families_without_a_device_filler_are_refused(api):
    lib = api._lib.load()
    out = api.device_words(64)
    ev = torch.zeros((1, 64), dtype=torch.int64, device="cuda")
    for family in (12, 13, 14, 15):
        assert lib.sp1hip_tracegen_riscv_field_chip(family, api._dptr(out), 32, api._dptr(ev), 1, None) == api._lib.ERROR_INVALID_ARGUMENT
        assert ("family %d" % family).encode() in lib.sp1hip_last_error()
    for kind in ("ed_add", "ed_decompress", "uint256_ops"):
        with pytest.raises(ValueError):
            api.tracegen_riscv_field_chip(kind, ev, 32)


# ---------------------------------------------------------------------------------------------------------- the native program
@pytest.mark.parametrize("kind", C.LARGE_KINDS)
def test_the_native_programs_device_form_equals_its_host_form(kind, tmp_path):
    assert os.path.exists(C.EXE), "tests/native/field_chip_rows is not built: run __graft_entry__.build()"
    n, height = C.LARGE
    ev = C.events(kind, n)
    msg = C.first_difference(kind, C.run_rows("host", kind, ev, height, tmp_path), C.run_rows("device", kind, ev, height, tmp_path), n)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------------------------ the shards
PROGRAMS = [(C.curve_program, "Secp256r1"), (C.curve_program, "Bn254"), (C.curve_program, "Bls12381"), (C.tower_program, "Bn254"), (C.tower_program, "Bls12381")]


@pytest.fixture(scope="module")
def program_events():
    """{kind: the executor's events} of the curve and tower programs run six times over: 6 additions, 12 doublings, 24 Fp calls (add,
    mul, sub, mul six times), 12 Fp2 additions / subtractions, 6 Fp2 products."""
    out = {}
    for program, name in PROGRAMS:
        ex = X.Executor(program(name, 6), stdin=[])
        for rec in X.run_records(ex, 1 << 20):
            if rec.kind in C.KINDS:
                out[rec.kind] = np.ascontiguousarray(rec.events)
    assert set(out) == set(C.KINDS)
    return out


def _host_chips(machine, tables):
    import core_real
    return [(a, i, core_real.to_col_major(tables[a.name][1].cuda()), core_real.to_col_major(tables[a.name][0].cuda()) if tables[a.name][0] is not None else None)
            for a, i in machine]


def _prep_of(chips):
    return {a.name: p for a, _, _, p in chips if p is not None}


def _assert_same_shard(host, device, n_events):
    """(machine, chips as ColMajor, publics, events [m, 11]) from the host tables against device_family_shard's return, word for word."""
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


def _both(kind, ev):
    machine, tables, publics, gev = MT.family_shard_from(kind, ev, "cpu")
    assert C.CHIPS[kind] in tables and "SyscallPrecompile" in tables
    chips = _host_chips(machine, tables)
    return (machine, chips, publics, gev), X.device_family_shard(kind, ev, _prep_of(chips), RT.RunContext())


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("n", SHARD_CALLS)
def test_device_family_shard_equals_the_host_shard(api, program_events, kind, n):
    ev = program_events[kind][:n]
    assert ev.shape == (n, C.event_words(kind))
    host, device = _both(kind, ev)
    _assert_same_shard(host, device, int(host[3].shape[0]))


@pytest.mark.parametrize("kind,n", PROOFS)
def test_the_proof_is_the_same_bytes_from_device_and_host_tables(api, program_events, kind, n):
    ev = program_events[kind][:n]
    if kind.endswith("_fp"):
        assert len(set((ev[:, 3] & 0xFF).tolist())) == 3            # add, mul, sub: three system calls in one shard
    host, device = _both(kind, ev)
    assert _prove(api, device[1], device[2]) == _prove(api, host[1], host[2])


# -------------------------------------------------------------------------------------------------------------- whole programs
def _no_host_tables(monkeypatch):
    def no_tracer(*args, **kwargs):
        raise AssertionError("a host tracer was asked for a table")
    monkeypatch.setattr(X.EventTracer, "__init__", no_tracer)
    for name in ("global_chip", "byte_range_tables", "fill_cluster"):
        monkeypatch.setattr(RT.Tracer, name, no_tracer)
    for name in ("memory_shard_from", "_close_precompile_shard", "family_shard_from"):
        monkeypatch.setattr(MT, name, no_tracer)


@pytest.mark.parametrize("program,name,want", [(C.curve_program, "Secp256r1", ["core", "secp256r1_add", "secp256r1_double", "memory"]),
                                               (C.tower_program, "Bls12381", ["core", "bls12381_fp", "bls12381_fp2_addsub", "bls12381_fp2_mul", "memory"])])
def test_a_hand_assembled_program_with_every_shard_made_on_the_device(api, program, name, want, monkeypatch):
    import core_real
    _no_host_tables(monkeypatch)
    ex = X.Executor(program(name), stdin=[])
    prep, kinds, pvs, gevs, entry = None, [], [], [], None
    for rec in X.run_records(ex, 1 << 20):
        assert rec.kind in X.DEVICE_SHARD_KINDS + X.DEVICE_FAMILY_KINDS, rec.kind
        if prep is None:
            prep = {n: core_real.to_col_major(t) for n, t in X.preprocessed_tables(ex, "cuda").items()}
        if rec.kind == "core":
            entry = rec.executed.pc_start if entry is None else entry
        machine, chips, publics, gev9 = X.device_shard_of(ex, rec, prep)
        assert frozenset(a.name for a, _ in machine) in RT.chip_clusters() and [c[0].name for c in chips] == [a.name for a, _ in machine]
        if rec.kind in X.DEVICE_FAMILY_KINDS:
            chip = X.FAMILIES[rec.kind][1]
            main = {c[0].name: c[2] for c in chips}[chip]
            assert main.height == RT.pad32(len(rec.events)) and main.width == R.chip(chip)[0].main_width
        kinds.append(rec.kind)
        pvs.append([int(v) for v in publics])
        gevs.append(X.global_events_11(gev9).cpu())
    assert kinds == want and ex.halted
    assert not X.global_events_balance(gevs + [X.image_events(ex)])
    # the public values chain from the entry point to HALT: every check of the reference's verifier up to the one a program that
    # halts without COMMIT cannot pass (tests/test_riscv_exec.py::run_program)
    vk_digest = X.verifying_key_words(ex, entry, "cuda")[3:]
    assert PVM.verify_proof_public_values([pvs[i] for i in X.proof_order(kinds)], entry, vk_digest) == "prev_commit_syscall doesn't equal the previous shard's commit_syscall"
    gm = {int(r[0]): int(r[2]) & C.M64 for r in ex.global_memory()}
    at = lambda off, n: sum(gm[C.DATA + off + 8 * k] << (64 * k) for k in range(n))
    if program is C.curve_program:
        p, a, nl = M.CURVES[name][:3]
        n, g = nl // 8, C.GENERATORS[name]
        g2 = C.affine_add(g, g, p, a)
        g3 = C.affine_add(g, g2, p, a)
        assert (at(0, n), at(8 * n, n)) == g2 and (at(16 * n, n), at(24 * n, n)) == C.affine_add(g3, g3, p, a)
    else:
        p, nl = M.FP_FIELDS[name][:2]
        n, slot = nl // 8, nl
        a_, b_ = (3 ** 200 + 12345) % p, p - 7
        c0, c1, d0, d1 = 5 ** 150 % p, p - 1, 7 ** 130 % p, 11 ** 100 % p
        el = lambda k: at(k * slot, n)
        assert el(0) == (a_ + b_) % p and el(2) == a_ * a_ % p and el(3) == (a_ - b_) % p and el(4) == b_ * ((a_ + b_) % p) % p
        assert (el(5), el(6)) == ((c0 * d0 - c1 * d1) % p, (c0 * d1 + c1 * d0) % p)
        assert (el(9), el(10)) == ((c0 + d0) % p, (c1 + d1) % p) and (el(11), el(12)) == ((c0 - d0) % p, (c1 - d1) % p)
