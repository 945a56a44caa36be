"""CPU: the ABI of the Keccak chips' device trace generation (sp1hip_tracegen_riscv_keccak / _keccak_control) as far as it goes
without a device — the width queries against the transcribed chips, and the argument checks, which answer before any launch."""
import ctypes as C

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_widths_are_the_transcribed_chips(lib):
    assert lib.sp1hip_tracegen_riscv_keccak_width() == 2640 == R.chip("KeccakPermute")[0].main_width
    assert lib.sp1hip_tracegen_riscv_keccak_control_width() == 634 == R.chip("KeccakPermuteControl")[0].main_width


@pytest.mark.parametrize("n,height", [(1, 23), (2, 32), (3, 64), (178956971, 32)])         # the last: 24 n wraps 32 bits
def test_permute_needs_24_rows_per_event(lib, n, height):
    assert 24 * n > height
    assert lib.sp1hip_tracegen_riscv_keccak(FAKE, height, FAKE, n, None) == BAD
    assert b"sp1hip_tracegen_riscv_keccak" in lib.sp1hip_last_error()


@pytest.mark.parametrize("n,height", [(1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)])
def test_control_needs_a_row_per_event(lib, n, height):
    assert lib.sp1hip_tracegen_riscv_keccak_control(FAKE, height, FAKE, n, None) == BAD
    assert b"sp1hip_tracegen_riscv_keccak_control" in lib.sp1hip_last_error()


@pytest.mark.parametrize("fn", ["sp1hip_tracegen_riscv_keccak", "sp1hip_tracegen_riscv_keccak_control"])
def test_null_pointers_only_with_nothing_to_do(lib, fn):
    f = getattr(lib, fn)
    assert f(None, 32, None, 0, None) == BAD                 # a null table with rows to write
    assert f(None, 32, FAKE, 1, None) == BAD
    assert f(FAKE, 32, None, 1, None) == BAD                 # null events with events to read
    assert f(None, 0, None, 0, None) == _lib.SUCCESS         # height 0: nothing to write, no launch
    assert f(FAKE, 0, FAKE, 0, None) == _lib.SUCCESS
    assert f(None, 0, None, 1, None) == BAD                  # ... but still no room for an event
