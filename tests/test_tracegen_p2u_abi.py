"""CPU: the ABI of the Poseidon2 and Uint256MulMod trace generators as far as it goes without a device — the symbols and their width
queries against the transcribed chips, the argument checks, which answer before any launch and name the function, and the agreement
of the header, the ctypes bindings, the generated Rust declarations, INTEGRATION.md and the Python tables (api.RISCV_TRACEGEN,
api.WORD_DESCRIPTORS, riscv_exec.DEVICE_WORD_KINDS / DEVICE_SHARD_KINDS)."""
import ctypes as C
import os
import re

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_more as M

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# chip: (entry point, u64 words of an event record, width)
ENTRIES = {"Poseidon2": ("sp1hip_tracegen_riscv_poseidon2", 26, 348), "Uint256MulMod": ("sp1hip_tracegen_riscv_uint256_mul", 31, 371)}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _refused(lib, fn, *args):
    assert getattr(lib, fn)(*args) == BAD, (fn, args)
    assert fn.encode() in lib.sp1hip_last_error()


@pytest.mark.parametrize("chip", sorted(ENTRIES))
def test_symbols_and_widths_are_the_transcribed_chips(lib, chip):
    fn, _, width = ENTRIES[chip]
    assert getattr(lib, fn + "_width")() == R.chip(chip)[0].main_width == width
    assert getattr(lib, fn) is not None


@pytest.mark.parametrize("chip", sorted(ENTRIES))
def test_argument_checks_answer_before_any_launch(lib, chip):
    fn, _, _ = ENTRIES[chip]
    for n, height in ((1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)):                                 # more events than rows
        _refused(lib, fn, FAKE, height, FAKE, n, None)
    for table, height, events, n in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1)):
        _refused(lib, fn, table, height, events, n, None)
    call = getattr(lib, fn)
    assert call(None, 0, None, 0, None) == _lib.SUCCESS                                              # height 0: nothing to write, no launch
    assert call(FAKE, 0, FAKE, 0, None) == _lib.SUCCESS


def test_the_header_the_bindings_and_the_rust_declarations_agree():
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    for chip, (fn, words, width) in ENTRIES.items():
        args = re.search(r"\bint %s\(([^)]*)\);" % fn, header).group(1).split(",")
        assert len(args) == len(bound[fn]) == 5, fn
        assert re.search(r"pub fn %s\(d_table: \*mut u32, height: u32, d_events: \*const u64, n_events: u32, stream: Stream\) -> c_int;" % fn, rust), fn
        assert re.search(r"\bint %s_width\(void\);\s*/\* %d \*/" % (fn, width), header), fn
        assert bound[fn + "_width"] == [] and "pub fn %s_width() -> c_int;" % fn in rust
        assert "pub fn %s(" % fn in integration and str(width) in integration, fn
    assert re.search(r"#define SP1HIP_RV64_POSEIDON2_WORDS 26\b", header) and re.search(r"#define SP1HIP_RV64_UINT256_WORDS 31\b", header)


def test_the_python_tables():
    from sp1_amd import api
    for chip, (fn, words, _) in ENTRIES.items():
        assert api.RISCV_TRACEGEN[chip] == (fn, words, None), chip
    assert (api.POSEIDON2_EVENT_WORDS, api.UINT256_EVENT_WORDS) == (X.POSEIDON2_WORDS, X.UINT256_WORDS) == (26, 31)
    assert api.WORD_DESCRIPTORS == {"poseidon2": (26, 0x33, -1, ((1, 8, 2, 18, 0),)),
                                    "uint256": (31, 0x1D, 2, ((1, 4, 3, 27, 1), (2, 8, 11, None, 0)))}
    assert api.WORD_DESCRIPTORS["poseidon2"][1] == M.SYS_POSEIDON2 and api.WORD_DESCRIPTORS["uint256"][1] == M.SYS_UINT256_MUL
    assert not set(api.WORD_DESCRIPTORS) & (set(api.PRECOMPILE_DESCRIPTORS) | set(api.SHA_DESCRIPTORS))
    assert X.DEVICE_WORD_KINDS == ("poseidon2", "uint256")
    assert X.DEVICE_SHARD_KINDS == X.DEVICE_KINDS + X.DEVICE_WORD_KINDS and not set(X.DEVICE_KINDS) & set(X.DEVICE_WORD_KINDS)
    assert set(X.DEVICE_SHARD_KINDS) == {"core", "memory"} | set(X.PRECOMPILE_KINDS)                # every kind the executor records
    for kind in X.DEVICE_WORD_KINDS:
        assert X._precompile_descriptor(kind) == api.WORD_DESCRIPTORS[kind]
    for kind in X.DEVICE_PRECOMPILE_KINDS:
        assert X._precompile_descriptor(kind) == api.PRECOMPILE_DESCRIPTORS[kind]
    for kind in X.DEVICE_SHA_KINDS:
        assert X._precompile_descriptor(kind) == api.SHA_DESCRIPTORS[kind]
    for name in ("tracegen_riscv_poseidon2", "tracegen_riscv_uint256_mul"):
        assert callable(getattr(api, name))


def test_device_shard_names_every_kind_it_makes():
    class Rec:
        kind = "bn254_fp"
    with pytest.raises(ValueError) as err:
        X.device_shard(None, Rec(), None)
    assert all(kind in str(err.value) for kind in X.DEVICE_SHARD_KINDS)
