"""CPU: the ABI of the Weierstrass and Fp / Fp2 trace generators as far as it goes without a device — the symbols and the width query
against the transcribed chips, the argument checks, which answer before any launch and name the function (and, for a family without
a device filler, the family), and the agreement of the header, the ctypes bindings, the generated Rust declarations, INTEGRATION.md
and the Python tables (api.FIELD_CHIP_KINDS, api.FAMILY_DESCRIPTORS, riscv_exec.DEVICE_FAMILY_KINDS, device_shard_of)."""
import ctypes as C
import os
import re

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R
from sp1_amd.machines import riscv_exec as X
from sp1_amd.machines import riscv_more as M
from sp1_amd.machines import riscv_more_trace as MT

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FN = "sp1hip_tracegen_riscv_field_chip"
CODED = "sp1hip_tracegen_riscv_syscall_precompile_coded"
WIDTHS = (1599, 1591, 1599, 1591, 2399, 2391, 306, 450, 592, 880, 1095, 1639)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _refused(lib, fn, *args):
    assert getattr(lib, fn)(*args) == BAD, (fn, args)
    assert fn.encode() in lib.sp1hip_last_error()


def test_widths_are_the_transcribed_chips(lib):
    kinds = list(X.FAMILIES)
    for family, width in enumerate(WIDTHS):
        assert kinds[family] == X.DEVICE_FAMILY_KINDS[family] and X.FAMILIES[kinds[family]][0] == family
        assert lib.sp1hip_tracegen_riscv_field_chip_width(family) == R.chip(X.FAMILIES[kinds[family]][1])[0].main_width == width
    for family in (12, 13, 14, 15, 2 ** 32 - 1):
        assert lib.sp1hip_tracegen_riscv_field_chip_width(family) == -1


def test_argument_checks_answer_before_any_launch(lib):
    call = lib.sp1hip_tracegen_riscv_field_chip
    for family in range(12):
        for n, height in ((1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)):                             # more events than rows
            _refused(lib, FN, family, FAKE, height, FAKE, n, None)
        for table, height, events, n in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1)):
            _refused(lib, FN, family, table, height, events, n, None)
        assert call(family, None, 0, None, 0, None) == _lib.SUCCESS                                  # height 0: nothing to write, no launch
        assert call(family, FAKE, 0, FAKE, 0, None) == _lib.SUCCESS
    for family in (12, 13, 14, 15, 2 ** 32 - 1):                                                     # no device filler: refused, and named
        for args in ((FAKE, 32, FAKE, 1), (None, 0, None, 0)):
            _refused(lib, FN, family, *args, None)
            assert ("family %d" % family).encode() in lib.sp1hip_last_error()


def test_the_coded_syscall_precompile_checks_its_arguments(lib):
    for words, code_word, arg2 in ((1, 0, -1), (65537, 3, -1), (44, 44, 2), (44, 3, 44), (44, 3, -2)):
        _refused(lib, CODED, FAKE, 32, FAKE, 1, words, code_word, arg2, None, None)
    _refused(lib, CODED, FAKE, 32, FAKE, 33, 44, 3, 2, None, None)
    _refused(lib, CODED, None, 32, FAKE, 1, 44, 3, 2, None, None)
    assert lib.sp1hip_tracegen_riscv_syscall_precompile_coded(None, 0, None, 0, 44, 3, 2, None, None) == _lib.SUCCESS


def test_the_header_the_bindings_and_the_rust_declarations_agree():
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    args = re.search(r"\bint %s\(([^)]*)\);" % FN, header).group(1).split(",")
    assert len(args) == len(bound[FN]) == 6
    decl = "pub fn %s(family: u32, d_table: *mut u32, height: u32, d_events: *const u64, n_events: u32, stream: Stream) -> c_int;" % FN
    assert decl in rust and decl in integration
    assert re.search(r"\bint %s_width\(uint32_t family\);" % FN, header) and bound[FN + "_width"] == [C.c_uint32]
    decl = "pub fn %s_width(family: u32) -> c_int;" % FN
    assert decl in rust and decl in integration
    args = re.search(r"\bint %s\(([^)]*)\);" % CODED, header).group(1).split(",")
    plain = re.search(r"\bint sp1hip_tracegen_riscv_syscall_precompile\(([^)]*)\);", header).group(1).split(",")
    assert len(args) == len(plain) == len(bound[CODED]) == 9 and bound[CODED] == bound["sp1hip_tracegen_riscv_syscall_precompile"]
    decl = ("pub fn %s(d_table: *mut u32, height: u32, d_events: *const u64, n_events: u32, words_per_event: u32, code_word: u32, arg2_word: i32, "
            "d_global_events: *mut i32, stream: Stream) -> c_int;" % CODED)
    assert decl in rust and decl in integration
    for width in WIDTHS:
        assert str(width) in integration and str(width) in header
    for family, kind in enumerate(X.DEVICE_FAMILY_KINDS):
        assert re.search(r"#define SP1HIP_RV64_FAMILY_%s %d\b" % (kind.upper(), family), header), kind


def test_the_python_tables():
    from sp1_amd import api
    source = open(os.path.join(ROOT, "sp1_amd", "csrc", "rv64_exec.cpp")).read()
    family_words = [int(v) for v in re.search(r"FAMILY_WORDS\[N_FAMILIES\] = \{([^}]*)\}", source).group(1).split(",")]
    assert X.DEVICE_FAMILY_KINDS == tuple(X.FAMILIES)[:12] == tuple(api.FIELD_CHIP_KINDS) == tuple(api.FAMILY_DESCRIPTORS)
    assert set(X.FAMILIES) - set(X.DEVICE_FAMILY_KINDS) == {"ed_add", "ed_decompress", "uint256_ops"}
    assert api.FAMILY_CODE_WORD == 3
    for kind in X.DEVICE_FAMILY_KINDS:
        family, chip = X.FAMILIES[kind]
        chip_name, shape, names, nw = MT.FAMILY_SHAPES[kind]
        words, syscall_id, arg2_word, segments = api.FAMILY_DESCRIPTORS[kind]
        assert api.FIELD_CHIP_KINDS[kind][:3] == (family, nw, len(names)) and chip_name == chip
        assert words == family_words[family] == 4 + (5 if len(names) == 2 else 3) * nw, kind
        if len(names) == 2:
            assert arg2_word == 2 and segments == ((1, nw, 4, 4 + 4 * nw, 1), (2, nw, 4 + 2 * nw, None, 0)), kind
        else:
            assert arg2_word == -1 and segments == ((1, nw, 4, 4 + 2 * nw, 0),), kind
        assert X.PRECOMPILES[kind] == (chip, None, 1, sum(s[1] for s in segments)), kind
        field = next(c for c in ("Secp256r1", "Bn254", "Bls12381") if chip.startswith(c))
        want = {"curve_add": lambda: M.CURVE_SYSCALLS[field][0], "curve_double": lambda: M.CURVE_SYSCALLS[field][1], "fp": lambda: None,
                "fp2_addsub": lambda: None, "fp2_mul": lambda: M.FP_SYSCALLS[field][5]}[shape]()
        assert syscall_id == want, kind
    assert not set(api.FAMILY_DESCRIPTORS) & (set(api.PRECOMPILE_DESCRIPTORS) | set(api.SHA_DESCRIPTORS) | set(api.WORD_DESCRIPTORS))
    for name in ("tracegen_riscv_field_chip", "tracegen_riscv_syscall_precompile_coded"):
        assert callable(getattr(api, name))
    with pytest.raises(ValueError) as err:
        api.tracegen_riscv_field_chip("ed_add", None, 32)
    assert "ed_add" in str(err.value)


def test_the_earlier_kinds_are_unchanged():
    assert X.DEVICE_SHARD_KINDS == X.DEVICE_KINDS + X.DEVICE_WORD_KINDS == ("core", "memory", "keccak", "secp256k1_add", "secp256k1_double", "sha_extend",
                                                                           "sha_compress", "poseidon2", "uint256")
    assert not set(X.DEVICE_SHARD_KINDS) & set(X.DEVICE_FAMILY_KINDS)


def test_device_shard_of_names_every_kind_it_makes():
    class Rec:
        kind = "ed_add"
    for kind in ("ed_add", "ed_decompress", "uint256_ops"):
        Rec.kind = kind
        with pytest.raises(ValueError) as err:
            X.device_shard_of(None, Rec(), None)
        assert kind in str(err.value) and all(k in str(err.value) for k in X.DEVICE_SHARD_KINDS + X.DEVICE_FAMILY_KINDS)
    with pytest.raises(ValueError) as err:
        X.device_family_shard("ed_add", None, None, None)
    assert all(k in str(err.value) for k in X.DEVICE_FAMILY_KINDS)
