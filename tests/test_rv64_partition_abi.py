"""CPU: the ABI of sp1hip_rv64_partition_* and of sp1hip_tracegen_riscv_syscall_instrs, _syscall_core, _state_bump and _memory_bump as
far as it goes without a device — the sizes and widths, the argument checks, which answer before any launch and name the function,
and the agreement of the header, the ctypes bindings and the generated Rust declarations."""
import ctypes as C
import os
import re

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null, 16-byte aligned pointer no check may follow: every call below returns before touching a device
ODD = C.c_void_p(0x1008)           # 8-byte aligned only
CHIPS = {"SyscallInstrs": ("syscall_instrs", 65), "SyscallCore": ("syscall_core", 10), "StateBump": ("state_bump", 14), "MemoryBump": ("memory_bump", 15)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _header():
    return open(os.path.join(ROOT, "include", "sp1hip.h")).read()


def test_scratch_size_and_constants(lib):
    header = _header()
    wg = int(re.search(r"#define SP1HIP_RV64_PARTITION_WORKGROUP (\d+)", header).group(1))
    assert int(re.search(r"#define SP1HIP_RV64_BINS (\d+)", header).group(1)) == 29
    assert int(re.search(r"#define SP1HIP_RV64_PARTITION_SCAN_SLICES (\d+)", header).group(1)) == 32
    for n in (0, 1, wg - 1, wg, wg + 1, 33 * wg, (1 << 30)):
        assert lib.sp1hip_rv64_partition_scratch_bytes(n) == max(-(-n // wg), 1) * 32 * 4, n
    enum = dict((k, int(v)) for k, v in re.findall(r"SP1HIP_RV64_BIN_(\w+) = (\d+)", header))
    assert enum == {"ALU": 0, "MEM": 14, "DIVIDE": 23, "X0": 24, "SYSCALL_INSTRS": 25, "SYSCALL_CORE": 26, "STATE_BUMP": 27, "MEMORY_BUMP": 28}


def test_partition_checks_its_arguments_before_any_launch(lib):
    count, scatter = lib.sp1hip_rv64_partition_count, lib.sp1hip_rv64_partition_scatter
    for args in ((None, 1, FAKE, FAKE), (FAKE, 1, None, FAKE), (FAKE, 1, FAKE, None), (FAKE, (1 << 30) + 1, FAKE, FAKE), (ODD, 1, FAKE, FAKE),
                 (FAKE, 1, C.c_void_p(0x1002), FAKE), (FAKE, 1, FAKE, C.c_void_p(0x1001))):
        assert count(*args, None) == BAD, args
        assert b"sp1hip_rv64_partition_count" in lib.sp1hip_last_error()
    for args in ((None, 1, FAKE, FAKE, FAKE, 11), (FAKE, 1, None, FAKE, FAKE, 11), (FAKE, 1, FAKE, None, FAKE, 11), (FAKE, 1, FAKE, FAKE, None, 11),
                 (FAKE, (1 << 30) + 1, FAKE, FAKE, FAKE, 11), (ODD, 1, FAKE, FAKE, FAKE, 11), (FAKE, 1, FAKE, FAKE, C.c_void_p(0x1004), 11),
                 (FAKE, 0, FAKE, FAKE, None, 11)):
        assert scatter(*args, None) == BAD, args
        assert b"sp1hip_rv64_partition_scatter" in lib.sp1hip_last_error()
    # no event: nothing to do, no launch
    assert count(None, 0, None, None, None) == _lib.SUCCESS and count(FAKE, 0, FAKE, FAKE, None) == _lib.SUCCESS
    assert scatter(None, 0, None, None, None, 0, None) == _lib.SUCCESS and scatter(FAKE, 0, FAKE, FAKE, FAKE, 44, None) == _lib.SUCCESS


def _call(lib, name, table, height, records, n, events=None):
    fn = getattr(lib, "sp1hip_tracegen_riscv_" + CHIPS[name][0])
    return fn(table, height, records, n, events, None) if name == "SyscallCore" else fn(table, height, records, n, None)


def _refused(lib, name, *args):
    assert _call(lib, name, *args) == BAD, (name, args)
    assert ("sp1hip_tracegen_riscv_" + CHIPS[name][0]).encode() in lib.sp1hip_last_error()


def test_widths_are_the_transcribed_chips(lib):
    for name, (fn, width) in CHIPS.items():
        assert getattr(lib, "sp1hip_tracegen_riscv_%s_width" % fn)() == width == R.chip(name)[0].main_width, name


@pytest.mark.parametrize("name", CHIPS)
@pytest.mark.parametrize("n,height", [(1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)])
def test_a_record_needs_a_row(lib, name, n, height):
    _refused(lib, name, FAKE, height, FAKE, n)
    if name == "SyscallCore":
        _refused(lib, name, FAKE, height, FAKE, n, FAKE)


@pytest.mark.parametrize("name", CHIPS)
def test_null_pointers_only_with_nothing_to_do(lib, name):
    for args in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1), (None, 0, None, 1)):
        _refused(lib, name, *args)
    assert _call(lib, name, None, 0, None, 0) == _lib.SUCCESS          # height 0: nothing to write, no launch
    assert _call(lib, name, FAKE, 0, FAKE, 0) == _lib.SUCCESS
    if name == "SyscallCore":
        assert _call(lib, name, FAKE, 0, FAKE, 0, FAKE) == _lib.SUCCESS
        _refused(lib, name, None, 32, FAKE, 1, FAKE)
        _refused(lib, name, FAKE, 32, None, 1, FAKE)


def test_the_header_the_bindings_and_the_rust_declarations_agree():
    header = _header()
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    for fn, _ in CHIPS.values():
        run, width = "sp1hip_tracegen_riscv_" + fn, "sp1hip_tracegen_riscv_%s_width" % fn
        args = re.search(r"\bint %s\(([^)]*)\);" % run, header).group(1).split(",")
        assert len(args) == len(bound[run]) == (6 if fn == "syscall_core" else 5), run
        assert re.search(r"\bint %s\(void\);" % width, header) and bound[width] == []
        assert "pub fn %s(" % run in rust and "pub fn %s() -> c_int;" % width in rust
        assert ("const sp1hip_rv64_alu_event_t* d_events" in args[2]) == fn.startswith("syscall")
    assert "pub fn sp1hip_rv64_partition_scratch_bytes(n_events: u64) -> u64;" in rust
    assert re.search(r"pub fn sp1hip_rv64_partition_count\(d_events: \*const u64, n_events: u64, d_scratch: \*mut u32, d_counts: \*mut u32, "
                     r"stream: Stream\) -> c_int;", rust)
    assert re.search(r"pub fn sp1hip_rv64_partition_scatter\(d_events: \*const u64, n_events: u64, d_scratch: \*const u32, d_counts: \*const u32, "
                     r"d_records: \*mut u64, records_words: u64, stream: Stream\) -> c_int;", rust)
    assert len(bound["sp1hip_rv64_partition_count"]) == 5 and len(bound["sp1hip_rv64_partition_scatter"]) == 7
    assert "pub const SP1HIP_RV64_BIN_MEMORY_BUMP: c_int = 28;" in rust
    # the earlier chip numbers stay as they are
    assert len(re.findall(r"SP1HIP_RV64_CHIP_\w+ = \d+", header)) == 14 and len(re.findall(r"SP1HIP_RV64_MEM_CHIP_\w+ = \d+", header)) == 9
