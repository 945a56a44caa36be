"""CPU: the ABI of the six later instruction chips of sp1hip_tracegen_riscv_alu (Bitwise, Lt, ShiftLeft, UType, Jal, Jalr: chip values
8-13) as far as it goes without a device — the width queries against the transcribed chips, and the argument checks, which answer
before any launch."""
import ctypes as C
import os
import re

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
NEW = {"Bitwise": (8, 51), "Lt": (9, 44), "ShiftLeft": (10, 65), "UType": (11, 31), "Jal": (12, 31), "Jalr": (13, 35)}
KINDS = [k for k, _ in NEW.values()]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_widths_are_the_transcribed_chips(lib):
    for name, (kind, width) in NEW.items():
        assert lib.sp1hip_tracegen_riscv_alu_width(kind) == width == R.chip(name)[0].main_width, name
    assert lib.sp1hip_tracegen_riscv_alu_width(14) == -1
    assert lib.sp1hip_tracegen_riscv_alu_width(99) == -1
    assert lib.sp1hip_tracegen_riscv_alu_width(-1) == -1


def test_an_unknown_chip_is_refused(lib):
    for kind in (14, 99, -1):
        assert lib.sp1hip_tracegen_riscv_alu(kind, FAKE, 32, FAKE, 1, None) == BAD
        assert b"sp1hip_tracegen_riscv_alu" in lib.sp1hip_last_error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,height", [(1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)])
def test_an_event_needs_a_row(lib, kind, n, height):
    assert lib.sp1hip_tracegen_riscv_alu(kind, FAKE, height, FAKE, n, None) == BAD
    assert b"sp1hip_tracegen_riscv_alu" in lib.sp1hip_last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_null_pointers_only_with_nothing_to_do(lib, kind):
    f = lib.sp1hip_tracegen_riscv_alu
    assert f(kind, None, 32, None, 0, None) == BAD                 # a null table with rows to write
    assert f(kind, None, 32, FAKE, 1, None) == BAD
    assert f(kind, FAKE, 32, None, 1, None) == BAD                 # null events with events to read
    assert f(kind, None, 0, None, 0, None) == _lib.SUCCESS         # height 0: nothing to write, no launch
    assert f(kind, FAKE, 0, FAKE, 0, None) == _lib.SUCCESS
    assert f(kind, None, 0, None, 1, None) == BAD                  # ... but still no room for an event


def test_the_header_and_the_bindings_agree():
    from sp1_amd import api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sp1hip.h")).read()
    bound = {name for name, _, _ in _lib.PROTOTYPES}
    for fn in ("sp1hip_tracegen_riscv_alu", "sp1hip_tracegen_riscv_alu_width"):
        assert re.search(r"\bint %s\(" % fn, header) and fn in bound
    enum = dict((n, int(v)) for n, v in re.findall(r"SP1HIP_RV64_CHIP_(\w+) = (\d+)", header))
    snake = lambda name: re.sub(r"(?<=[a-z])(?=[A-Z])", "_", name).upper()
    assert {snake(n): k for n, k in api.RISCV_ALU_CHIPS.items()} == enum
    for name, (kind, _) in NEW.items():
        assert api.RISCV_ALU_CHIPS[name] == kind == enum[snake(name)]
    rust = open(os.path.join(root, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    for name, k in enum.items():
        assert re.search(r"pub const SP1HIP_RV64_CHIP_%s: c_int = %d;" % (name, k), rust), name
