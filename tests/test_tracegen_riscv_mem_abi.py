"""CPU: the ABI of sp1hip_tracegen_riscv_mem (the nine load and store chips: LoadByte, LoadHalf, LoadWord, LoadDouble, LoadX0,
StoreByte, StoreHalf, StoreWord, StoreDouble) as far as it goes without a device — the width queries against the transcribed chips,
and the argument checks, which answer before any launch."""
import ctypes as C
import os
import re

import pytest

from sp1_amd import _lib
from sp1_amd.machines import riscv as R

BAD = _lib.ERROR_INVALID_ARGUMENT
FAKE = C.c_void_p(0x1000)          # a non-null pointer no check may follow: every call below must return before touching a device
CHIPS = {"LoadByte": (0, 47), "LoadHalf": (1, 44), "LoadWord": (2, 44), "LoadDouble": (3, 39), "LoadX0": (4, 48), "StoreByte": (5, 50),
         "StoreHalf": (6, 45), "StoreWord": (7, 44), "StoreDouble": (8, 39)}
KINDS = [k for k, _ in CHIPS.values()]
FN = b"sp1hip_tracegen_riscv_mem"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_widths_are_the_transcribed_chips(lib):
    for name, (kind, width) in CHIPS.items():
        assert lib.sp1hip_tracegen_riscv_mem_width(kind) == width == R.chip(name)[0].main_width == R.RECORDED[name][0], name
    for kind in (9, 99, -1):
        assert lib.sp1hip_tracegen_riscv_mem_width(kind) == -1


def test_an_unknown_chip_is_refused(lib):
    for kind in (9, 99, -1):
        assert lib.sp1hip_tracegen_riscv_mem(kind, FAKE, 32, FAKE, 1, None) == BAD
        assert FN in lib.sp1hip_last_error()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,height", [(1, 0), (33, 32), (2 ** 32 - 1, 2 ** 32 - 2)])
def test_an_event_needs_a_row(lib, kind, n, height):
    assert lib.sp1hip_tracegen_riscv_mem(kind, FAKE, height, FAKE, n, None) == BAD
    assert FN in lib.sp1hip_last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_null_pointers_only_with_nothing_to_do(lib, kind):
    f = lib.sp1hip_tracegen_riscv_mem
    for args in ((None, 32, None, 0), (None, 32, FAKE, 1), (FAKE, 32, None, 1), (None, 0, None, 1)):
        # a null table with rows to write; null events with events to read; height 0 with an event: no room for it
        assert f(kind, args[0], args[1], args[2], args[3], None) == BAD, args
        assert FN in lib.sp1hip_last_error()
    assert f(kind, None, 0, None, 0, None) == _lib.SUCCESS         # height 0: nothing to write, no launch
    assert f(kind, FAKE, 0, FAKE, 0, None) == _lib.SUCCESS


def test_the_header_and_the_bindings_agree():
    from sp1_amd import api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "sp1hip.h")).read()
    bound = {name: args for name, _, args in _lib.PROTOTYPES}
    for fn in ("sp1hip_tracegen_riscv_mem", "sp1hip_tracegen_riscv_mem_width"):
        assert re.search(r"\bint %s\(" % fn, header) and fn in bound
    assert len(bound["sp1hip_tracegen_riscv_mem"]) == 6 and len(bound["sp1hip_tracegen_riscv_mem_width"]) == 1
    enum = dict((n, int(v)) for n, v in re.findall(r"SP1HIP_RV64_MEM_CHIP_(\w+) = (\d+)", header))
    snake = lambda name: re.sub(r"(?<=[a-z])(?=[A-Z])", "_", name).upper()
    assert {snake(n): k for n, k in api.RISCV_MEM_CHIPS.items()} == enum
    for name, (kind, _) in CHIPS.items():
        assert api.RISCV_MEM_CHIPS[name] == kind == enum[snake(name)]
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    fields = re.search(r"typedef struct \{ uint64_t ([\w, ]+); \}\s*sp1hip_rv64_mem_event_t;", plain).group(1).split(", ")
    assert fields == [n for n, _ in _lib.Rv64MemEvent._fields_] and C.sizeof(_lib.Rv64MemEvent) == 96 == 8 * api.MEM_EVENT_WORDS
    rust = open(os.path.join(root, "rust", "sp1-hip-sys", "src", "lib.rs")).read()
    for name, k in enum.items():
        assert re.search(r"pub const SP1HIP_RV64_MEM_CHIP_%s: c_int = %d;" % (name, k), rust), name
    assert "pub fn sp1hip_tracegen_riscv_mem(" in rust and "pub struct Sp1HipRv64MemEvent" in rust


def test_the_event_struct_has_the_layout_of_its_ctypes_mirror(tmp_path):
    """tests/test_abi.py compiles every struct of the header that its own list names and compares sizes and offsets with the ctypes
    mirrors; sp1hip_rv64_mem_event_t is not in that list (a comment stands between the brace and the name in the header, so that
    test's search for struct names passes it by), so the same check for it is made here."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cls, cname = _lib.Rv64MemEvent, "sp1hip_rv64_mem_event_t"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sp1hip.h"', 'int main(void) {', 'printf("size %%zu\\n", sizeof(%s));' % cname]
    lines += ['printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f) for f, _ in cls._fields_]
    lines.append('return 0; }')
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("size")) == C.sizeof(cls) == 96
    assert {k: int(v) for k, v in got.items()} == {f: getattr(cls, f).offset for f, _ in cls._fields_}
