"""CPU: the ABI of sp1hip_tracegen_riscv_memory_global, _syscall_precompile and sp1hip_precompile_local_records as far as it goes
without a device — the width queries against the transcribed chips, the argument checks, which answer before any launch and name
the function, the agreement of the header, the ctypes bindings and the generated Rust declarations — and riscv_exec.program_shards:
on a small guest with secp256k1 calls, a fibonacci run of three core shards and the Keccak, Poseidon2 and SHA-2 guests it yields,
table for table, what it yielded when one generator cut the run and built the tables (digests taken on those revisions), so does
host_shard mapped over run_records, and run_records' records hold the raw inputs from which the host builders make exactly those
shards, cut without a table being built."""
import ctypes as C
import hashlib
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sp1_amd import _lib  # noqa: E402
from sp1_amd.machines import riscv as R  # noqa: E402

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _refused(lib, fn, *args):
    assert getattr(lib, fn)(*args) == BAD, (fn, args)
    assert fn.encode() in lib.sp1hip_last_error()


def test_widths_are_the_transcribed_chips(lib):
    from sp1_amd import api
    assert lib.sp1hip_tracegen_riscv_memory_global_width() == 30 == api.MEMORY_GLOBAL_WIDTH
    assert R.chip("MemoryGlobalInit")[0].main_width == R.chip("MemoryGlobalFinalize")[0].main_width == 30
    assert lib.sp1hip_tracegen_riscv_syscall_precompile_width() == 10 == api.SYSCALL_PRECOMPILE_WIDTH == R.chip("SyscallPrecompile")[0].main_width
    assert api.MEMORY_GLOBAL_RECORD_WORDS == 3 and api.MEMORY_GLOBAL_KINDS == {"init": 0, "finalize": 1}


@pytest.mark.parametrize("finalize", [0, 1])
def test_memory_global_argument_checks(lib, finalize):
    fn = "sp1hip_tracegen_riscv_memory_global"
    for n, height in ((1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)):                       # a record needs a row
        _refused(lib, fn, finalize, FAKE, height, FAKE, n, 0, None, None)
        _refused(lib, fn, finalize, FAKE, height, FAKE, n, 0, FAKE, None)
    for table, height, records, n in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1), (None, 0, None, 1)):
        _refused(lib, fn, finalize, table, height, records, n, 8, None, None)
        _refused(lib, fn, finalize, table, height, records, n, 8, FAKE, None)
    call = lib.sp1hip_tracegen_riscv_memory_global
    assert call(finalize, None, 0, None, 0, 0, None, None) == _lib.SUCCESS               # height 0: nothing to write, no launch
    assert call(finalize, FAKE, 0, FAKE, 0, 2 ** 48 - 8, FAKE, None) == _lib.SUCCESS
    _refused(lib, fn, 2 + finalize, FAKE, 0, FAKE, 0, 0, None, None)                       # the kind is 0 or 1
    _refused(lib, fn, -1, FAKE, 0, FAKE, 0, 0, None, None)


def test_syscall_precompile_argument_checks(lib):
    fn = "sp1hip_tracegen_riscv_syscall_precompile"
    for n, height in ((1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)):
        _refused(lib, fn, FAKE, height, FAKE, n, 77, 9, -1, None, None)
    for table, height, events, n in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1), (None, 0, None, 1)):
        _refused(lib, fn, table, height, events, n, 77, 9, -1, FAKE, None)
    for words, syscall_id, arg2 in ((1, 9, -1), (0, 9, -1), (65537, 9, -1), (43, 256, 2), (43, 10, 43), (43, 10, -2)):
        _refused(lib, fn, FAKE, 0, FAKE, 0, words, syscall_id, arg2, None, None)           # the event's shape, even with nothing to do
    call = lib.sp1hip_tracegen_riscv_syscall_precompile
    assert call(None, 0, None, 0, 77, 9, -1, None, None) == _lib.SUCCESS
    assert call(FAKE, 0, FAKE, 0, 43, 10, 2, FAKE, None) == _lib.SUCCESS


def test_precompile_local_records_argument_checks(lib):
    fn = "sp1hip_precompile_local_records"
    seg = lambda *rows: np.array(rows, dtype=np.uint32).reshape(-1)
    ptr = lambda a: a.ctypes.data_as(U32)
    keccak, none = seg((1, 25, 2, 52, 1)), 0xFFFFFFFF
    _refused(lib, fn, FAKE, 1 << 20, FAKE, 1, 77, None, 1, None)                           # no segments
    _refused(lib, fn, FAKE, 1 << 20, FAKE, 1, 77, ptr(keccak), 0, None)
    five = seg(*[(1, 1, 2, none, 0)] * 5)
    _refused(lib, fn, FAKE, 1 << 20, FAKE, 1, 77, ptr(five), 5, None)                      # more than four
    for bad in ((77, 25, 2, 52, 1), (1, 0, 2, 52, 1), (1, 25, 28, 52, 1), (1, 25, 2, 53, 1), (1, 25, 77, none, 1), (1, 78, 2, none, 1),
                (1, 25, 0xFFFFFFF0, none, 1), (1, 0x80000000, 2, none, 1)):
        _refused(lib, fn, FAKE, 1 << 20, FAKE, 1, 77, ptr(seg(bad)), 1, None)              # a segment reads behind the event record
    _refused(lib, fn, FAKE, 1 << 20, FAKE, 1, 1, ptr(keccak), 1, None)
    _refused(lib, fn, FAKE, 24, FAKE, 1, 77, ptr(keccak), 1, None)                          # 25 records do not fit
    _refused(lib, fn, None, 25, FAKE, 1, 77, ptr(keccak), 1, None)
    _refused(lib, fn, FAKE, 25, None, 1, 77, ptr(keccak), 1, None)
    _refused(lib, fn, FAKE, 2 ** 40, FAKE, 2 ** 32 - 1, 77, ptr(keccak), 1, None)          # too many records for one launch
    call = lib.sp1hip_precompile_local_records
    assert call(None, 0, None, 0, 77, ptr(keccak), 1, None) == _lib.SUCCESS                # no call: nothing to write, no launch
    add = seg((1, 8, 3, 35, 1), (2, 8, 19, none, 0))
    assert call(FAKE, 0, FAKE, 0, 43, ptr(add), 2, None) == _lib.SUCCESS


def test_the_header_the_bindings_and_the_rust_declarations_agree():
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    for run, count in (("sp1hip_tracegen_riscv_memory_global", 8), ("sp1hip_tracegen_riscv_syscall_precompile", 9), ("sp1hip_precompile_local_records", 8)):
        args = re.search(r"\bint %s\(([^)]*)\);" % run, header).group(1).split(",")
        assert len(args) == len(bound[run]) == count, run
        assert "pub fn %s(" % run in rust
    for width in ("sp1hip_tracegen_riscv_memory_global_width", "sp1hip_tracegen_riscv_syscall_precompile_width"):
        assert re.search(r"\bint %s\(void\);" % width, header) and bound[width] == [] and "pub fn %s() -> c_int;" % width in rust
    assert re.search(r"pub fn sp1hip_tracegen_riscv_memory_global\(finalize: c_int, d_table: \*mut u32, height: u32, d_records: \*const u64, "
                     r"n_records: u32, previous_addr: u64, d_global_events: \*mut i32, stream: Stream\) -> c_int;", rust)
    # records and segments are plain words: no struct was added for them
    assert not re.search(r"}\s*sp1hip_\w*(memory_global|precompile|segment)\w*_t\s*;", header)


# ------------------------------------------------------------------------------ program_shards, run_records and host_shard
def _guest():
    """2G, G + 2G, 6G by the secp256k1 precompiles from a hand-assembled program (the program of test_gpu_tracegen_secp.py): a core
    shard, a secp256k1_add shard, a secp256k1_double shard and a memory shard."""
    import rv_asm as A
    import secp_cases as SC
    from sp1_amd.machines import riscv_exec as X
    words = lambda v: b"".join(struct.pack("<Q", (v >> (64 * i)) & SC.M64) for i in range(4))
    data = words(SC.G[0]) + words(SC.G[1]) + words(SC.G[0]) + words(SC.G[1])
    prog = A.li(28, 0x78100000)
    prog += [A.enc("addi", 10, 28, 0), A.enc("addi", 11, 0, 0)] + A.li(5, 0x0000010B) + [A.enc("ecall")]
    prog += [A.enc("addi", 10, 28, 64), A.enc("addi", 11, 28, 0)] + A.li(5, 0x0001010A) + [A.enc("ecall")]
    prog += [A.enc("addi", 10, 28, 64), A.enc("addi", 11, 0, 0)] + A.li(5, 0x0000010B) + [A.enc("ecall")]
    return X.Executor(A.elf(prog + A.halt(0), data=data + bytes(32)), stdin=[])


def _digest_of(shard):
    """One shard as program_shards yields it -> sha256 over its kind, chip names, every table, the public values and the events."""
    kind, machine, tables, publics, gev, sh = shard
    h = hashlib.sha256(kind.encode())
    for a, _ in machine:
        prep, main = tables[a.name]
        h.update(a.name.encode())
        for t in (prep, main):
            h.update(b"-" if t is None else np.ascontiguousarray(t.cpu().numpy(), dtype=np.int64).tobytes() + str(tuple(t.shape)).encode())
    h.update(np.ascontiguousarray(publics.cpu().numpy(), dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(gev.cpu().numpy(), dtype=np.int64).tobytes())
    h.update(b"core" if sh is not None else b"none")
    return h.hexdigest()


def _guest_file(name, stdin):
    from sp1_amd.machines import riscv_exec as X
    return X.Executor(X.guest_file(name + ".elf"), stdin=[stdin])


# run: (executor, max_cycles) — the hand-assembled guest above, the multi-core-shard run of test_public_values._fibonacci_shards (the
# `prev` chain across core shards), and the Keccak, Poseidon2 and SHA-2 guests sized as in test_riscv_exec.py (their adapters)
RUNS = {"secp256k1": (_guest, 1 << 20),
        "fibonacci": (lambda: _guest_file("fibonacci", struct.pack("<Q", 300)), 3000),
        "keccak": (lambda: _guest_file("keccak", bytes(300)), 4000),
        "poseidon2": (lambda: _guest_file("poseidon2", struct.pack("<Q", 20)), 1 << 20),
        "sha2": (lambda: _guest_file("sha2", bytes(range(200))), 8000)}


def program_shards_digests(run="secp256k1"):
    from sp1_amd.machines import riscv_exec as X
    guest, max_cycles = RUNS[run]
    return [(s[0], _digest_of(s)) for s in X.program_shards(guest(), max_cycles)]


def host_shard_digests(run):
    """The same over run_records and host_shard: what program_shards is made of."""
    from sp1_amd.machines import riscv_exec as X
    guest, max_cycles = RUNS[run]
    ex = guest()
    return [(r.kind, _digest_of((r.kind, *X.host_shard(ex, r), r.executed))) for r in X.run_records(ex, max_cycles)]


# program_shards_digests() on the revision before program_shards could yield a shard untraced
BEFORE = [("core", "c04d98c1764ebab57fcdbd5e46e82107abc28df73b99928128241af7529af777"),
          ("secp256k1_add", "11e252049056ec3ac2d059c817a7c50b788f684d66ce718edd1d64e591e056fa"),
          ("secp256k1_double", "07c3b09736e2e558c81f64de0c54613463126e7ec9f2db9b9887efe8b199b372"),
          ("memory", "a1c289ec9343181b51efdd93761e451de4a809cfa39def4dcf84c7eed442e684")]
# program_shards_digests(run) on 119a32c, the last revision whose program_shards cut the run and built the tables in one generator
PINNED = {
    "secp256k1": BEFORE,
    "fibonacci": [("core", "629c8cab4401b9988e92f2d80ee90c411d18b43002355cef0854b6db3811f767"),
                  ("core", "f81cc83dfa012945774fae61d9caac66bc3b0837c8b66b26ec7b4929e8c84a29"),
                  ("core", "f4e643e7691404010ee00d818778a69725f046306f10ccd3360717d968220627"),
                  ("memory", "8c519c1cb4cc1064c63b8795a3d2c657c04ace843c823f402f85f55e53b97a1f")],
    "keccak": [("core", "e6783fdb681508d0c2d3b786899b24474337fe8e7a71007735c49f299142ff89"),
               ("core", "d7a946cd6392627a3c4a988638c7176b68940f56a1bd2a7e8351b637d1d61bff"),
               ("core", "18a1831162ce91ce88ddec817779c62d652746471f0b0f0c49ee6c0072d5624c"),
               ("keccak", "7eb13ba9c7ae7ef627c77aeafaf46cea147e00b5789da754e8d73f143697547d"),
               ("memory", "c840cc1e4bd9fcc29c130ad86f474d8943c3f77011ec0f6b952b0ff9dd43f1db")],
    "poseidon2": [("core", "a53e967a266629e2b6779b3ffdb097ad6672a0ad208c185809b52561d360b169"),
                  ("poseidon2", "851d940bb2231cfd788171e9749c0cef7994fff26b0f43034ef708a4f58a7817"),
                  ("sha_extend", "99887a901635362e8f202aa4e2d47244ba0bfc409d6e5ffeecd8e9f74a198555"),
                  ("sha_compress", "0c3a191228f564ca02a69c0e34dcd3aa8e0b98fec89a263c7e707b11313ed7e0"),
                  ("memory", "0c7a143d916c7c28165c0b9fb4c7f785a26d6d0e26459c5936f3e8ff9ae378ff")],
    "sha2": [("core", "16141d1dd39a0c1ca5acaf038a86298582d524cd20aae5b271b1d80cc352915f"),
             ("core", "7552471eb5f3ff20d15e71aee5729891cf84550ddb197270718e05970e8cb9d1"),
             ("sha_extend", "69170ddafd6ab425e724dc07e6f6c6c417a777f4d6f9a3dfd9c26211b46178df"),
             ("sha_compress", "984b940bfe2c2639a557984df0d594f506d35d4ccccefbd64a7d941c115d3924"),
             ("memory", "0f3143f5b11d77a573bd1d3adbd78d116c7a66c547f9557f244e468c306db293")],
}


def test_program_shards_with_the_flags_off_is_what_it_was():
    assert program_shards_digests() == BEFORE
    assert host_shard_digests("secp256k1") == BEFORE


@pytest.mark.parametrize("run", [r for r in RUNS if r != "secp256k1"])
def test_program_shards_and_host_shard_over_run_records_are_what_program_shards_was(run):
    assert program_shards_digests(run) == PINNED[run]
    assert host_shard_digests(run) == PINNED[run]


def test_program_shards_with_the_flags_on_yields_the_builders_inputs():
    """A record's fields are exactly what the host builders are called with: building from them gives the traced shards."""
    from sp1_amd.machines import riscv_exec as X
    from sp1_amd.machines import riscv_more_trace as MT
    from sp1_amd.machines import riscv_trace as RT
    ex, seen = _guest(), []
    for rec in X.run_records(ex, 1 << 20):
        kind, ctx = rec.kind, rec.ctx
        assert isinstance(ctx, RT.RunContext)
        if kind == "core":
            assert rec.prev is None and rec.events is None
            seen.append((kind, _digest_of((kind, *X.host_shard(ex, rec), rec.executed))))
            continue
        assert rec.executed is None and rec.prev is None
        if kind == "memory":
            ia, ir, fa, fr, previous_init, previous_fin = rec.init_addrs, rec.init_recs, rec.fin_addrs, rec.fin_recs, rec.previous_init, rec.previous_fin
            assert (previous_init, previous_fin) == (0, 0) and len(fa) > len(ia) > 0 and ir.shape == (len(ia), 2) and fr.shape == (len(fa), 2)
            built = MT.memory_shard_from(ia, ir, fr, "cpu", previous_addr=previous_init, ctx=ctx, fin_addrs=fa, previous_fin_addr=previous_fin)
        else:
            raw = rec.events
            assert raw.dtype == np.int64 and raw.shape == ({"secp256k1_add": (1, 43), "secp256k1_double": (2, 26)}[kind])
            built = (MT.secp256k1_add_shard_from if kind == "secp256k1_add" else MT.secp256k1_double_shard_from)(raw, "cpu", ctx=ctx)
        seen.append((kind, _digest_of((kind,) + tuple(built) + (None,))))
    assert seen == BEFORE


def test_run_records_cuts_the_run_and_builds_no_table(monkeypatch):
    """The fibonacci run of three core shards, with every table maker patched to raise: run_records still yields every kind in order,
    core shard k's `prev` is execution_public_values chained over shards 0 .. k - 1, and core_limit=1 yields one core shard and the same
    memory records."""
    from sp1_amd.machines import riscv_exec as X
    from sp1_amd.machines import riscv_more_trace as MT

    def no_tables(*args, **kwargs):
        raise AssertionError("run_records asked for a table")
    monkeypatch.setattr(X.EventTracer, "__init__", no_tables)
    for name in [n for n in dir(MT) if n.endswith("_shard_from")] + ["_close_precompile_shard"]:
        monkeypatch.setattr(MT, name, no_tables)
    guest, max_cycles = RUNS["fibonacci"]
    records = list(X.run_records(guest(), max_cycles))
    assert [r.kind for r in records] == ["core", "core", "core", "memory"] and all(r.ctx is records[0].ctx for r in records)
    prev = None
    for r in records[:3]:
        assert (r.prev is None) == (prev is None) and (prev is None or np.array_equal(np.asarray(r.prev), np.asarray(prev)))
        assert r.events is None and r.executed.events.shape[0] > 0
        prev = X.execution_public_values(r.executed, prev)
    assert records[2].executed.halted and records[0].ctx.final[0] == records[2].executed.clk_end
    limited = list(X.run_records(guest(), max_cycles, core_limit=1))
    assert [r.kind for r in limited] == ["core", "memory"] and limited[0].prev is None
    fields = ("init_addrs", "init_recs", "fin_addrs", "fin_recs", "previous_init", "previous_fin")
    for name in fields:
        assert np.array_equal(getattr(limited[1], name), getattr(records[3], name)), name
    assert limited[1].ctx.final == records[3].ctx.final


def test_device_memory_shard_keeps_the_host_fillers_assertions():
    """Both are made in numpy before anything is uploaded: no device is needed to be refused."""
    import memory_global_cases as G
    from sp1_amd.machines import riscv_exec as X
    from sp1_amd.machines import riscv_trace as RT
    ctx, (fa, fr) = RT.RunContext(), G.records("continuing", "finalize", 33)
    none = (np.zeros(0, dtype=np.uint64), np.zeros((0, 2), dtype=np.int64))
    swapped = fa.copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    with pytest.raises(AssertionError, match="increase strictly"):
        X.device_memory_shard(*none, swapped, fr, {}, ctx, previous_fin=0x8000)
    with pytest.raises(AssertionError, match="increase strictly"):
        X.device_memory_shard(*none, fa, fr, {}, ctx, previous_fin=int(fa[0]))             # the first address equals the previous shard's last
    with pytest.raises(AssertionError, match="does not close its chain"):
        X.device_memory_shard(*none, fa[:1] * 0, fr[:1] * 0, {}, ctx)
