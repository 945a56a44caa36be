"""CPU: the ABI of the secp256k1 chips' device trace generation (sp1hip_tracegen_riscv_secp256k1_add / _double) as far as it goes
without a device — the width queries against the transcribed chips, and the argument checks, which answer before any launch."""
import ctypes as C

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
FNS = ["sp1hip_tracegen_riscv_secp256k1_add", "sp1hip_tracegen_riscv_secp256k1_double"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_widths_are_the_transcribed_chips(lib):
    assert lib.sp1hip_tracegen_riscv_secp256k1_add_width() == 1599 == R.chip("Secp256k1AddAssign")[0].main_width
    assert lib.sp1hip_tracegen_riscv_secp256k1_double_width() == 1591 == R.chip("Secp256k1DoubleAssign")[0].main_width


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("n,height", [(1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)])
def test_an_event_needs_a_row(lib, fn, n, height):
    assert getattr(lib, fn)(FAKE, height, FAKE, n, None) == BAD
    assert fn.encode() in lib.sp1hip_last_error()


@pytest.mark.parametrize("fn", FNS)
def test_null_pointers_only_with_nothing_to_do(lib, fn):
    f = getattr(lib, fn)
    assert f(None, 32, None, 0, None) == BAD                 # a null table with rows to write
    assert f(None, 32, FAKE, 1, None) == BAD
    assert f(FAKE, 32, None, 1, None) == BAD                 # null events with events to read
    assert f(None, 0, None, 0, None) == _lib.SUCCESS         # height 0: nothing to write, no launch
    assert f(FAKE, 0, FAKE, 0, None) == _lib.SUCCESS
    assert f(None, 0, None, 1, None) == BAD                  # ... but still no room for an event


def test_the_header_and_the_bindings_agree():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sp1hip.h")).read()
    bound = {name for name, _, _ in _lib.PROTOTYPES}
    for fn in FNS + [f + "_width" for f in FNS]:
        assert re.search(r"\bint %s\(" % fn, header) and fn in bound
