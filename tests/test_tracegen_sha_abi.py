"""CPU: the ABI of the four SHA-256 trace generators as far as it goes without a device — the symbols and their width queries against
the transcribed chips, the argument checks, which answer before any launch and name the function, the quad segment form's bounds
check in sp1hip_precompile_local_records, and the agreement of the header, the ctypes bindings, the generated Rust declarations and
the Python tables (api.RISCV_TRACEGEN, api.SHA_DESCRIPTORS, riscv_exec.DEVICE_KINDS)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_more as M

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = C.POINTER(C.c_uint32)
# chip: (entry point, u64 words of an event record, rows per call)
ENTRIES = {"ShaExtend": ("sp1hip_tracegen_riscv_sha_extend", 786, 48), "ShaExtendControl": ("sp1hip_tracegen_riscv_sha_extend_control", 786, 1),
           "ShaCompress": ("sp1hip_tracegen_riscv_sha_compress", 155, 80), "ShaCompressControl": ("sp1hip_tracegen_riscv_sha_compress_control", 155, 1)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _refused(lib, fn, *args):
    assert getattr(lib, fn)(*args) == BAD, (fn, args)
    assert fn.encode() in lib.sp1hip_last_error()


@pytest.mark.parametrize("chip", sorted(ENTRIES))
def test_symbols_and_widths_are_the_transcribed_chips(lib, chip):
    fn, _, _ = ENTRIES[chip]
    assert getattr(lib, fn + "_width")() == R.chip(chip)[0].main_width
    assert getattr(lib, fn) is not None


@pytest.mark.parametrize("chip", sorted(ENTRIES))
def test_argument_checks_answer_before_any_launch(lib, chip):
    fn, _, rows = ENTRIES[chip]
    for n, height in ((1, 0), (33, 32 * rows), (2 ** 32 - 1, 2 ** 32 - 2), (1, rows - 1)):           # a call's rows need the height
        _refused(lib, fn, FAKE, height, FAKE, n, None)
    for table, height, events, n in ((None, 32 * rows, None, 0), (None, 32 * rows, FAKE, 1), (FAKE, 32 * rows, None, 1)):
        _refused(lib, fn, table, height, events, n, None)
    call = getattr(lib, fn)
    assert call(None, 0, None, 0, None) == _lib.SUCCESS                                              # height 0: nothing to write, no launch
    assert call(FAKE, 0, FAKE, 0, None) == _lib.SUCCESS


def test_the_quad_segment_forms_bounds(lib):
    fn = "sp1hip_precompile_local_records"
    seg = lambda *rows: np.array(rows, dtype=np.uint32).reshape(-1)
    ptr = lambda a: a.ctypes.data_as(U32)
    quad, none = 0xFFFFFFFE, 0xFFFFFFFF
    for bad in ((1, 64, 531, quad, 0), (1, 65, 530, quad, 0), (1, 197, 0, quad, 0), (786, 1, 0, quad, 0), (1, 0, 530, quad, 0), (1, 64, 0xFFFFFFF0, quad, 0),
                (1, 0x40000000, 0, quad, 0)):
        _refused(lib, fn, FAKE, 1 << 20, FAKE, 1, 786, ptr(seg(bad)), 1, None)         # pairs_word + 4 count > words_per_event
    _refused(lib, fn, FAKE, 63, FAKE, 1, 786, ptr(seg((1, 64, 530, quad, 0))), 1, None)  # 64 records do not fit
    call = lib.sp1hip_precompile_local_records
    assert call(FAKE, 0, FAKE, 0, 786, ptr(seg((1, 64, 530, quad, 0))), 1, None) == _lib.SUCCESS     # no call: no launch
    assert call(FAKE, 0, FAKE, 0, 786, ptr(seg((1, 196, 2, quad, 0))), 1, None) == _lib.SUCCESS      # 2 + 4 * 196 = 786: the last word
    assert call(FAKE, 0, FAKE, 0, 155, ptr(seg((2, 8, 3, 147, 2), (1, 64, 19, none, 1))), 2, None) == _lib.SUCCESS
    # the pair form's bound did not move: 530 + 2 * 128 = 786 fits, one more word does not
    assert call(FAKE, 0, FAKE, 0, 786, ptr(seg((1, 128, 530, none, 0))), 1, None) == _lib.SUCCESS
    _refused(lib, fn, FAKE, 1 << 20, FAKE, 1, 786, ptr(seg((1, 128, 531, none, 0))), 1, None)


def test_the_header_the_bindings_and_the_rust_declarations_agree():
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    for chip, (fn, _, _) in ENTRIES.items():
        args = re.search(r"\bint %s\(([^)]*)\);" % fn, header).group(1).split(",")
        assert len(args) == len(bound[fn]) == 5, fn
        assert re.search(r"pub fn %s\(d_table: \*mut u32, height: u32, d_events: \*const u64, n_events: u32, stream: Stream\) -> c_int;" % fn, rust), fn
        assert re.search(r"\bint %s_width\(void\);\s*/\* %d \*/" % (fn, R.chip(chip)[0].main_width), header), fn
        assert bound[fn + "_width"] == [] and "pub fn %s_width() -> c_int;" % fn in rust
        assert "pub fn %s(" % fn in integration, fn
    assert "0xFFFFFFFE" in header


def test_the_python_tables():
    from sp1_amd import api
    for chip, (fn, words, _) in ENTRIES.items():
        assert api.RISCV_TRACEGEN[chip] == (fn, words, None), chip
    assert (api.SHA_EXTEND_EVENT_WORDS, api.SHA_COMPRESS_EVENT_WORDS) == (X.SHA_EXTEND_WORDS, X.SHA_COMPRESS_WORDS) == (786, 155)
    assert set(api.SHA_DESCRIPTORS) == {"sha_extend", "sha_compress"}
    assert api.SHA_DESCRIPTORS["sha_extend"][:2] == (X.SHA_EXTEND_WORDS, M.SYS_SHA_EXTEND)
    assert api.SHA_DESCRIPTORS["sha_compress"][:2] == (X.SHA_COMPRESS_WORDS, M.SYS_SHA_COMPRESS)
    assert not set(api.SHA_DESCRIPTORS) & set(api.PRECOMPILE_DESCRIPTORS)
    assert X.DEVICE_SHA_KINDS == ("sha_extend", "sha_compress")
    assert set(X.DEVICE_KINDS) == {"core", "memory"} | set(X.DEVICE_PRECOMPILE_KINDS) | set(X.DEVICE_SHA_KINDS)
    assert len(X.DEVICE_KINDS) == 2 + len(X.DEVICE_PRECOMPILE_KINDS) + len(X.DEVICE_SHA_KINDS)
    for name in ("tracegen_riscv_sha_extend", "tracegen_riscv_sha_extend_control", "tracegen_riscv_sha_compress", "tracegen_riscv_sha_compress_control"):
        assert callable(getattr(api, name))
