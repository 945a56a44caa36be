"""CPU: the ABI of the device count of the Byte, Range and Program multiplicities (sp1hip_lookup_count_sends, _count_program,
_counts_finish) as far as it goes without a device — the symbols, the prototypes in the header, the ctypes bindings and the Rust
declarations, and the argument checks, which answer before any launch: a malformed description, null buffers, a stride of 0."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from sp1_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lookup_count_cases as LC  # noqa: E402

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
FNS = {"sp1hip_lookup_count_sends": 12, "sp1hip_lookup_count_program": 9, "sp1hip_lookup_counts_finish": 5}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _sends(lib, words, main_width, prep_width, main, prep, rows, byte=FAKE, rng=FAKE, status=FAKE):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    ptr = words.ctypes.data_as(C.POINTER(C.c_uint32)) if words.size else None
    return lib.sp1hip_lookup_count_sends(ptr, words.size, main_width, prep_width, main, prep, rows, byte, rng, status, 0, None)


def test_the_header_the_bindings_and_the_rust_declarations_agree(lib):
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    for fn, n_args in FNS.items():
        proto = re.search(r"\bint %s\(([^;]*)\);" % fn, plain)
        assert proto and len(proto.group(1).split(",")) == n_args == len(bound[fn]), fn
        assert getattr(lib, fn).restype is C.c_int
        assert "pub fn %s(" % fn in rust, fn
    protos = "".join(re.findall(r"\bint sp1hip_lookup_\w+\([^;]*\);", plain))
    assert set(re.findall(r"\b\w+_t\b", protos)) == {"uint32_t", "uint64_t", "sp1hip_stream_t"}  # plain pointers and integers, no struct


@pytest.mark.parametrize("name", sorted(LC.malformed()))
def test_a_malformed_description_is_refused_before_any_launch(lib, name):
    words, main_width, prep_width = LC.malformed()[name]
    assert _sends(lib, words, main_width, prep_width, FAKE, FAKE, 32) == BAD
    assert b"sp1hip_lookup_count_sends" in lib.sp1hip_last_error()
    assert _sends(lib, words, main_width, prep_width, FAKE, FAKE, 0) == BAD                      # also with nothing to count


def test_values_outside_the_field_are_refused(lib):
    good = LC.message_chip().to_array().copy()
    for at in (5, 8):                                  # the first form's constant, its first term's weight
        words = good.copy()
        words[at] = LC.P
        assert _sends(lib, words, 6, 0, FAKE, None, 32) == BAD, at


def test_null_buffers_only_with_nothing_to_read(lib):
    words = LC.message_chip().to_array()
    prep_words = LC.message_chip(prep_columns=True).to_array()
    assert _sends(lib, words, 6, 0, None, None, 32) == BAD                                       # rows to read and no table
    assert _sends(lib, prep_words, 6, 2, FAKE, None, 32) == BAD
    for null in ("byte", "rng", "status"):
        assert _sends(lib, words, 6, 0, FAKE, None, 32, **{null: None}) == BAD, null
    assert _sends(lib, words, 6, 0, FAKE, None, 2 ** 30 + 1) == BAD                              # taller than any table
    assert b"sp1hip_lookup_count_sends" in lib.sp1hip_last_error()
    assert _sends(lib, words, 6, 0, None, None, 0) == _lib.SUCCESS                               # rows == 0: no launch
    assert _sends(lib, prep_words, 6, 2, None, None, 0) == _lib.SUCCESS
    assert _sends(lib, np.array([0], np.uint32), 0, 0, None, None, 32) == _lib.SUCCESS           # a chip that sends nothing: no launch
    receive_only = np.array([1, 0, 5, 4] + [0, 1] * 5, np.uint32)                                # one byte RECEIVE of constants
    assert _sends(lib, receive_only, 0, 0, None, None, 32) == _lib.SUCCESS


def test_program_count_arguments(lib):
    f = lib.sp1hip_lookup_count_program
    assert f(None, 20, 1, 0x200000, 4, FAKE, FAKE, 0, None) == BAD
    assert f(FAKE, 20, 1, 0x200000, 4, None, FAKE, 0, None) == BAD
    assert f(FAKE, 20, 1, 0x200000, 4, FAKE, None, 0, None) == BAD
    assert f(FAKE, 0, 1, 0x200000, 4, FAKE, FAKE, 0, None) == BAD
    assert f(FAKE, 4097, 1, 0x200000, 4, FAKE, FAKE, 0, None) == BAD
    assert b"sp1hip_lookup_count_program" in lib.sp1hip_last_error()
    assert f(None, 20, 0, 0x200000, 4, FAKE, FAKE, 0, None) == _lib.SUCCESS                      # nothing executed: no launch


def test_finish_arguments(lib):
    f = lib.sp1hip_lookup_counts_finish
    assert f(FAKE, 16, None, None, None) == BAD
    assert f(None, 16, None, FAKE, None) == BAD
    assert f(FAKE, 2 ** 32, None, FAKE, None) == BAD
    assert b"sp1hip_lookup_counts_finish" in lib.sp1hip_last_error()
