"""CPU: the ABI of sp1hip_tracegen_riscv_divrem, _alu_x0 and _memory_local as far as it goes without a device — the width queries
against the transcribed chips, the argument checks, which answer before any launch and name the function, and the agreement of the
header, the ctypes bindings and the generated Rust declarations."""
import ctypes as C
import os
import re

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
CHIPS = {"DivRem": ("divrem", 246), "AluX0": ("alu_x0", 34), "MemoryLocal": ("memory_local", 20)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _call(lib, name, table, height, records, n, events=None):
    fn = getattr(lib, "sp1hip_tracegen_riscv_" + CHIPS[name][0])
    return fn(table, height, records, n, events, None) if name == "MemoryLocal" else fn(table, height, records, n, None)


def _refused(lib, name, *args):
    assert _call(lib, name, *args) == BAD, (name, args)
    assert ("sp1hip_tracegen_riscv_" + CHIPS[name][0]).encode() in lib.sp1hip_last_error()


def test_widths_are_the_transcribed_chips(lib):
    for name, (fn, width) in CHIPS.items():
        assert getattr(lib, "sp1hip_tracegen_riscv_%s_width" % fn)() == width == R.chip(name)[0].main_width, name
    from sp1_amd import api
    assert api.MEMORY_LOCAL_WIDTH == 20 and api.MEMORY_LOCAL_RECORD_WORDS == 5 and api.GLOBAL_EVENT_WORDS == 9
    assert lib.sp1hip_tracegen_riscv_alu_width(14) == -1       # the new chips have no number at the older entry point


@pytest.mark.parametrize("name", CHIPS)
@pytest.mark.parametrize("n,height", [(1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)])
def test_a_record_needs_a_row(lib, name, n, height):
    _refused(lib, name, FAKE, height, FAKE, n)
    if name == "MemoryLocal":
        _refused(lib, name, FAKE, height, FAKE, n, FAKE)


@pytest.mark.parametrize("name", CHIPS)
def test_null_pointers_only_with_nothing_to_do(lib, name):
    for args in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1), (None, 0, None, 1)):
        # a null table with rows to write; null records with records to read; height 0 with a record: no room for it
        _refused(lib, name, *args)
    assert _call(lib, name, None, 0, None, 0) == _lib.SUCCESS          # height 0: nothing to write, no launch
    assert _call(lib, name, FAKE, 0, FAKE, 0) == _lib.SUCCESS
    if name == "MemoryLocal":
        assert _call(lib, name, FAKE, 0, FAKE, 0, FAKE) == _lib.SUCCESS
        _refused(lib, name, None, 32, FAKE, 1, FAKE)
        _refused(lib, name, FAKE, 32, None, 1, FAKE)


def test_the_header_the_bindings_and_the_rust_declarations_agree():
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    for fn, _ in CHIPS.values():
        run, width = "sp1hip_tracegen_riscv_" + fn, "sp1hip_tracegen_riscv_%s_width" % fn
        args = re.search(r"\bint %s\(([^)]*)\);" % run, header).group(1).split(",")
        assert len(args) == len(bound[run]) == (6 if fn == "memory_local" else 5), run
        assert re.search(r"\bint %s\(void\);" % width, header) and bound[width] == []
        assert "pub fn %s(" % run in rust and "pub fn %s() -> c_int;" % width in rust
        assert ("const sp1hip_rv64_alu_event_t* d_events" in args[2]) == (fn != "memory_local")
    assert "const uint64_t* d_records" in header and "int32_t* d_global_events" in header
    assert re.search(r"pub fn sp1hip_tracegen_riscv_memory_local\(d_table: \*mut u32, height: u32, d_records: \*const u64, n_records: u32, "
                     r"d_global_events: \*mut i32, stream: Stream\) -> c_int;", rust)
    assert re.search(r"pub fn sp1hip_tracegen_riscv_divrem\(d_table: \*mut u32, height: u32, d_events: \*const Sp1HipRv64AluEvent, n_events: u32, "
                     r"stream: Stream\) -> c_int;", rust)
    # no chip number and no struct was added for them
    assert len(re.findall(r"SP1HIP_RV64_CHIP_\w+ = \d+", header)) == 14 and not re.search(r"SP1HIP_RV64\w*_(DIVREM|DIV_REM|ALU_X0|MEMORY_LOCAL)", header)
