"""CPU: the ABI of sp1hip_tracegen_riscv_memory_global, _syscall_precompile and sp1hip_precompile_local_records as far as it goes
without a device — the width queries against the transcribed chips, the argument checks, which answer before any launch and name
the function, the agreement of the header, the ctypes bindings and the generated Rust declarations — and riscv_exec.program_shards
with the new flags off: on a small guest with secp256k1 calls it yields, table for table, what it yielded before the flags existed
(a digest taken on that revision), and with the flags on the raw inputs from which the host builders make exactly those shards."""
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


# ------------------------------------------------------------------------------------------------ program_shards, the flags off
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


def program_shards_digests(**flags):
    from sp1_amd.machines import riscv_exec as X
    return [(s[0], _digest_of(s)) for s in X.program_shards(_guest(), 1 << 20, **flags)]


# program_shards_digests() on the revision before the flags existed
BEFORE = [("core", "c04d98c1764ebab57fcdbd5e46e82107abc28df73b99928128241af7529af777"),
          ("secp256k1_add", "11e252049056ec3ac2d059c817a7c50b788f684d66ce718edd1d64e591e056fa"),
          ("secp256k1_double", "07c3b09736e2e558c81f64de0c54613463126e7ec9f2db9b9887efe8b199b372"),
          ("memory", "a1c289ec9343181b51efdd93761e451de4a809cfa39def4dcf84c7eed442e684")]


def test_program_shards_with_the_flags_off_is_what_it_was():
    assert program_shards_digests() == BEFORE
    assert program_shards_digests(untraced_memory=False, untraced_precompile=()) == BEFORE


def test_program_shards_with_the_flags_on_yields_the_builders_inputs():
    """The untraced tuples hold exactly what the host builders are called with: building from them gives the traced shards."""
    from sp1_amd.machines import riscv_exec as X
    from sp1_amd.machines import riscv_more_trace as MT
    from sp1_amd.machines import riscv_trace as RT
    seen = []
    for kind, machine, tables, ctx, gev, raw in X.program_shards(_guest(), 1 << 20, untraced_memory=True,
                                                                  untraced_precompile={"secp256k1_add", "secp256k1_double", "keccak"}):
        if kind == "core":
            seen.append((kind, _digest_of((kind, machine, tables, ctx, gev, raw))))
            continue
        assert machine is None and tables is None and gev is None and isinstance(ctx, RT.RunContext)
        if kind == "memory":
            ia, ir, fa, fr, previous_init, previous_fin = raw
            assert (previous_init, previous_fin) == (0, 0) and len(fa) > len(ia) > 0 and ir.shape == (len(ia), 2) and fr.shape == (len(fa), 2)
            built = MT.memory_shard_from(ia, ir, fr, "cpu", previous_addr=previous_init, ctx=ctx, fin_addrs=fa, previous_fin_addr=previous_fin)
        else:
            assert raw.dtype == np.int64 and raw.shape == ({"secp256k1_add": (1, 43), "secp256k1_double": (2, 26)}[kind])
            built = (MT.secp256k1_add_shard_from if kind == "secp256k1_add" else MT.secp256k1_double_shard_from)(raw, "cpu", ctx=ctx)
        seen.append((kind, _digest_of((kind,) + tuple(built) + (None,))))
    assert seen == BEFORE


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
