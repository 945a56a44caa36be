"""CPU: the ABI of the EdAddAssign, EdDecompress and Uint256Ops trace generators and of the touched words' records as far as it goes
without a device — the symbols and the width queries against the transcribed chips, the argument checks, which answer before any
launch and name the function, and the agreement of the header, the ctypes bindings, the generated Rust declarations, INTEGRATION.md
and the Python tables (api.FAMILY_REST_DESCRIPTORS, api.RISCV_TRACEGEN, riscv_exec.DEVICE_FAMILY_REST_KINDS, device_shard_any)."""
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
KINDS = ("ed_add", "ed_decompress", "uint256_ops")
FNS = {k: "sp1hip_tracegen_riscv_" + k for k in KINDS}
RECORDS = "sp1hip_precompile_touched_records"
WIDTHS = {"ed_add": 1347, "ed_decompress": 1123, "uint256_ops": 477}
WORDS = {"ed_add": 44, "ed_decompress": 24, "uint256_ops": 58}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _refused(lib, fn, *args):
    assert getattr(lib, fn)(*args) == BAD, (fn, args)
    assert fn.encode() in lib.sp1hip_last_error()


def test_widths_are_the_transcribed_chips(lib):
    for kind in KINDS:
        assert getattr(lib, FNS[kind] + "_width")() == R.chip(X.FAMILIES[kind][1])[0].main_width == WIDTHS[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_argument_checks_answer_before_any_launch(lib, kind):
    call = getattr(lib, FNS[kind])
    for n, height in ((1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)):                                 # more events than rows
        _refused(lib, FNS[kind], FAKE, height, FAKE, n, None)
    for table, height, events, n in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1)):
        _refused(lib, FNS[kind], table, height, events, n, None)
    assert call(None, 0, None, 0, None) == _lib.SUCCESS                                              # height 0: nothing to write, no launch
    assert call(FAKE, 0, FAKE, 0, None) == _lib.SUCCESS


def test_the_touched_records_check_their_arguments(lib):
    call = lib.sp1hip_precompile_touched_records
    for family in (0, 11, 12, 15, 2 ** 32 - 1):                                                      # ed_add (12) is two plain segments
        _refused(lib, RECORDS, FAKE, 1 << 20, FAKE, 1, family, None)
        assert b"13" in lib.sp1hip_last_error() and b"14" in lib.sp1hip_last_error()
    for family, per_call in ((13, 8), (14, 23)):
        _refused(lib, RECORDS, FAKE, 4 * per_call - 1, FAKE, 4, family, None)                        # no room for the last record
        _refused(lib, RECORDS, None, 4 * per_call, FAKE, 4, family, None)
        _refused(lib, RECORDS, FAKE, 4 * per_call, None, 4, family, None)
        _refused(lib, RECORDS, FAKE, 2 ** 40, FAKE, 2 ** 31 // per_call + 1, family, None)           # more than 2^31 - 1 records
        assert call(None, 0, None, 0, family, None) == _lib.SUCCESS                                  # no events: nothing to write, no launch
        assert call(FAKE, 100, FAKE, 0, family, None) == _lib.SUCCESS
    assert lib.sp1hip_precompile_local_records(FAKE, 100, FAKE, 1, 58, (C.c_uint32 * 25)(*([1, 1, 2, 0xFFFFFFFF, 0] * 5)), 5, None) == BAD   # still four segments


def test_the_header_the_bindings_and_the_rust_declarations_agree():
    header = open(os.path.join(ROOT, "include", "sp1hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    secp = re.search(r"\bint sp1hip_tracegen_riscv_secp256k1_add\(([^)]*)\);", header).group(1)
    for kind in KINDS:
        fn = FNS[kind]
        assert re.search(r"\bint %s\(([^)]*)\);" % fn, header).group(1) == secp                     # the shape of sp1hip_tracegen_riscv_secp256k1_add
        assert bound[fn] == bound["sp1hip_tracegen_riscv_secp256k1_add"] and len(bound[fn]) == 5
        decl = "pub fn %s(d_table: *mut u32, height: u32, d_events: *const u64, n_events: u32, stream: Stream) -> c_int;" % fn
        assert decl in rust and decl in integration
        assert re.search(r"\bint %s_width\(void\);" % fn, header) and bound[fn + "_width"] == []
        assert "pub fn %s_width() -> c_int;" % fn in rust
        assert str(WIDTHS[kind]) in integration and str(WIDTHS[kind]) in header
        assert re.search(r"#define SP1HIP_RV64_FAMILY_%s %d\b" % (kind.upper(), X.FAMILIES[kind][0]), header), kind
    args = re.search(r"\bint %s\(([^)]*)\);" % RECORDS, header).group(1).split(",")
    assert len(args) == len(bound[RECORDS]) == 6
    decl = "pub fn %s(d_records: *mut u64, records_capacity: u64, d_events: *const u64, n_events: u32, family: u32, stream: Stream) -> c_int;" % RECORDS
    assert decl in rust and decl in integration


def test_the_python_tables():
    from sp1_amd import api
    source = open(os.path.join(ROOT, "sp1_amd", "csrc", "rv64_exec.cpp")).read()
    family_words = [int(v) for v in re.search(r"FAMILY_WORDS\[N_FAMILIES\] = \{([^}]*)\}", source).group(1).split(",")]
    assert X.DEVICE_FAMILY_REST_KINDS == KINDS == tuple(X.FAMILIES)[12:] == tuple(api.FAMILY_REST_DESCRIPTORS)
    assert not set(api.FAMILY_REST_DESCRIPTORS) & (set(api.FAMILY_DESCRIPTORS) | set(api.PRECOMPILE_DESCRIPTORS) | set(api.SHA_DESCRIPTORS) | set(api.WORD_DESCRIPTORS))
    ids = {"ed_add": M.SYS_ED_ADD, "ed_decompress": M.SYS_ED_DECOMPRESS, "uint256_ops": None}
    assert (M.SYS_ED_ADD, M.SYS_ED_DECOMPRESS, M.SYS_UINT256_ADD_CARRY, M.SYS_UINT256_MUL_CARRY) == (0x07, 0x08, 0x30, 0x31) and api.FAMILY_CODE_WORD == 3
    for kind in KINDS:
        family, chip = X.FAMILIES[kind]
        words, syscall_id, arg2_word, local = api.FAMILY_REST_DESCRIPTORS[kind]
        assert MT.FAMILY_SHAPES[kind][0] == chip
        assert words == family_words[family] == WORDS[kind] and syscall_id == ids[kind] and arg2_word == 2, kind
        per_call = sum(s[1] for s in local) if kind == "ed_add" else api.TOUCHED_RECORDS_PER_CALL[local]
        registers = 3 if kind == "uint256_ops" else 0                 # x12, x13, x14: records, but no memory words of the split's cost
        assert X.PRECOMPILES[kind] == (chip, None, 1, per_call - registers), kind
        assert api.RISCV_TRACEGEN[chip] == (FNS[kind], words, None), kind
        assert callable(getattr(api, "tracegen_riscv_" + kind))
    assert api.FAMILY_REST_DESCRIPTORS["ed_add"][3] == ((1, 8, 4, 36, 1), (2, 8, 20, None, 0))
    assert api.FAMILY_REST_DESCRIPTORS["ed_decompress"][3] == 13 and api.FAMILY_REST_DESCRIPTORS["uint256_ops"][3] == 14
    with pytest.raises(ValueError) as err:
        api.precompile_touched_records(None, 12)
    assert "13" in str(err.value) and "14" in str(err.value)


def test_the_earlier_constants_are_unchanged():
    from sp1_amd import api
    assert X.DEVICE_SHARD_KINDS == X.DEVICE_KINDS + X.DEVICE_WORD_KINDS == ("core", "memory", "keccak", "secp256k1_add", "secp256k1_double", "sha_extend",
                                                                           "sha_compress", "poseidon2", "uint256")
    assert X.DEVICE_FAMILY_KINDS == tuple(X.FAMILIES)[:12] == tuple(api.FIELD_CHIP_KINDS) == tuple(api.FAMILY_DESCRIPTORS)
    assert X.DEVICE_ANY_KINDS == X.DEVICE_SHARD_KINDS + X.DEVICE_FAMILY_KINDS + X.DEVICE_FAMILY_REST_KINDS
    assert len(set(X.DEVICE_ANY_KINDS)) == len(X.DEVICE_ANY_KINDS) == 24
    assert set(X.DEVICE_ANY_KINDS) == {"core", "memory"} | set(X.PRECOMPILES)                        # every kind run_records can yield
    lib = _lib.load()
    assert [lib.sp1hip_tracegen_riscv_field_chip_width(f) for f in (12, 13, 14, 15)] == [-1] * 4     # the family entry point goes on refusing them


def test_device_shard_any_names_every_kind():
    class Rec:
        kind = "ed25519_verify"
    with pytest.raises(ValueError) as err:
        X.device_shard_any(None, Rec(), None)
    assert "ed25519_verify" in str(err.value) and all(k in str(err.value) for k in X.DEVICE_ANY_KINDS)
    with pytest.raises(ValueError) as err:
        X.device_family_rest_shard("bn254_add", None, None, None)
    assert "bn254_add" in str(err.value) and all(k in str(err.value) for k in X.DEVICE_FAMILY_REST_KINDS)
    for kind in KINDS:                                                                              # the earlier dispatcher is as it was
        Rec.kind = kind
        with pytest.raises(ValueError):
            X.device_shard_of(None, Rec(), None)
