"""GPU (-m gpu): device trace generation for the secp256k1 precompile chips (sp1hip_tracegen_riscv_secp256k1_add: Secp256k1AddAssign,
1,599 columns; sp1hip_tracegen_riscv_secp256k1_double: Secp256k1DoubleAssign, 1,591 columns) against the host filler of the same
events (riscv_more_trace.secp256k1_add_table / _double_table): every word of every column, padding rows included, bit for bit.
Shapes (events, height): (0, 32) padding only, (1, 32), (32, 32) no padding, (33, 64), (300, 320) across a 256-lane workgroup.
Events: the operand set of tests/secp_cases.py, cycled — the edge field elements in every ordered pair, multiples of G, random
elements; clocks on and next to a 2^24 boundary, pointers with full upper limbs and with a carry into the second limb. x3 / y3
are pinned independently of the filler by the words the events carry and, for multiples of G, by Python's affine arithmetic;
the native program's device forms (rows and fp256 alone) equal its host forms; and the two shards of a hand-assembled 2G,
G + 2G, 6G program check row by row with the device tables substituted and prove to the same bytes as from the host tables."""
import os
import struct
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import secp_cases as SC  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more_trace as MT  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

KINDS = ["add", "double"]


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


_MADE = {}


def _device_table(api, kind, n, height):
    """The device table of a shape as uint32 numpy [width, height], made once."""
    if (kind, n) not in _MADE:
        g = MT.secp256k1_device_table(kind, SC.events(kind, n), height)
        assert (g.width, g.height) == (R.chip(SC.CHIPS[kind])[0].main_width, height)
        _MADE[(kind, n)] = g.words.view(g.width, g.height).cpu().numpy().view(np.uint32)
    return _MADE[(kind, n)]


def test_widths(api):
    assert api._L().sp1hip_tracegen_riscv_secp256k1_add_width() == R.chip("Secp256k1AddAssign")[0].main_width
    assert api._L().sp1hip_tracegen_riscv_secp256k1_double_width() == R.chip("Secp256k1DoubleAssign")[0].main_width


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,height", SC.SHAPES)
def test_table_equals_the_host_filler(api, kind, n, height):
    want = SC.montgomery_col_major(SC.host_table(kind, n, height))
    msg = SC.first_difference(kind, want, _device_table(api, kind, n, height), n)
    assert msg is None, msg


@pytest.mark.parametrize("kind", KINDS)
def test_x3_y3_are_the_words_written_and_pythons_multiples_of_g(api, kind):
    n, height = SC.SHAPES[-1]
    got = _device_table(api, kind, n, height)
    u = SC.events(kind, n).view(np.uint64)
    written = [(sum(int(w) << (64 * i) for i, w in enumerate(r[-8:-4])), sum(int(w) << (64 * i) for i, w in enumerate(r[-4:]))) for r in u]
    assert SC.result_words(kind, got, range(n)) == written
    first = {"add": 111, "double": 110}[kind]                      # where the multiples of G begin in the operand set
    mg = SC.multiples_of_g(2 * SC.N_MULTIPLES + 1)
    if kind == "add":
        want = [SC.affine_add(mg[2 * SC.N_MULTIPLES], SC.G)] * SC.N_MULTIPLES              # (k + 1) G + (81 - k) G = 82 G
    else:
        want = [mg[2 * k + 1] for k in range(SC.N_MULTIPLES)]                              # 2 (k + 1) G
    assert SC.result_words(kind, got, range(first, first + SC.N_MULTIPLES)) == want


@pytest.mark.parametrize("kind", KINDS)
def test_native_device_form_equals_its_host_form(kind, tmp_path):
    assert os.path.exists(SC.EXE), "tests/native/secp_rows is not built: run __graft_entry__.build()"
    n, height = SC.SHAPES[-1]
    ev = SC.events(kind, n)
    host = SC.run_rows("host", kind, ev, height, tmp_path)
    dev = SC.run_rows("device", kind, ev, height, tmp_path)
    msg = SC.first_difference(kind, host, dev, n)
    assert msg is None, msg


def test_native_fp256_device_form_equals_its_host_form(tmp_path):
    """fp256 alone on the device — add, sub, mul, inv and the quotient modulo secp256k1's prime and, the modulus being data, bn254's
    — against the host form of the same record file, which tests/test_tracegen_secp_host.py pins to Python integers."""
    import test_tracegen_secp_host as H
    for name in ("secp256k1", "bn254"):
        p = H.MODULI[name]
        records = H.fp_records(p, 11)
        host = H._fp(records, p, tmp_path, "host")
        assert host == H.fp_expected(records, p)
        assert H._fp(records, p, tmp_path, "device") == host, name


def test_argument_checks(api):
    for fn, words in ((api.tracegen_riscv_secp256k1_add, 43), (api.tracegen_riscv_secp256k1_double, 26)):
        ev = torch.zeros((33, words), dtype=torch.int64, device="cuda")
        with pytest.raises(api._lib.Sp1HipError):
            fn(ev, 32)                                               # 33 rows do not fit
        with pytest.raises(api._lib.Sp1HipError):
            fn(ev[:1], 0)
        with pytest.raises(AssertionError):
            fn(ev[:, :words - 1].contiguous(), 64)                   # not this chip's event records
        assert fn(ev[:0], 0).words.numel() == 0


def _canonical_rows(col_major):
    """api.ColMajor (Montgomery words) -> canonical int64 [height, width] on the CPU."""
    w = col_major.words.view(col_major.width, col_major.height).cpu().to(torch.int64) & 0xFFFFFFFF
    return (w * pow(1 << 32, -1, RT.P) % RT.P).t().contiguous()


def test_both_shards_of_a_program_with_the_system_calls(api):
    """2G, G + 2G, 6G by the precompiles from a hand-assembled program (the program of test_riscv_exec.py's
    test_secp256k1_add_and_double_system_calls_and_their_shards): both shards' device tables equal the host ones (the written words
    come from the executor here), the shards with the device tables substituted check row by row, and their proofs are the same bytes."""
    import core_real
    import machine_check as MC
    import rv_asm as A
    from sp1_amd.machines import public_values as PVM
    words = lambda v: b"".join(struct.pack("<Q", (v >> (64 * i)) & SC.M64) for i in range(4))
    data = words(SC.G[0]) + words(SC.G[1]) + words(SC.G[0]) + words(SC.G[1])
    prog = A.li(28, 0x78100000)
    prog += [A.enc("addi", 10, 28, 0), A.enc("addi", 11, 0, 0)] + A.li(5, 0x0000010B) + [A.enc("ecall")]          # p = 2G
    prog += [A.enc("addi", 10, 28, 64), A.enc("addi", 11, 28, 0)] + A.li(5, 0x0001010A) + [A.enc("ecall")]        # q = G + 2G
    prog += [A.enc("addi", 10, 28, 64), A.enc("addi", 11, 0, 0)] + A.li(5, 0x0000010B) + [A.enc("ecall")]         # q = 6G
    ex = X.Executor(A.elf(prog + A.halt(0), data=data + bytes(32)), stdin=[])
    seen = []
    L, lsh, batch = 17, 12, 8
    for rec in X.run_records(ex, 1 << 20):
        kind, events = rec.kind, rec.events
        if not kind.startswith("secp256k1_"):
            continue
        machine, tabs, publics, gev = X.host_shard(ex, rec)
        short = kind[len("secp256k1_"):]
        chip = SC.CHIPS[short]
        assert events.shape == ({"add": 1, "double": 2}[short], SC.WORDS[short])
        host = tabs[chip][1]
        made = MT.secp256k1_device_table(short, events, int(host.shape[0]))
        want = core_real.to_col_major(host.cuda())
        msg = SC.first_difference(short, want.words.view(want.width, want.height).cpu().numpy().view(np.uint32),
                                  made.words.view(made.width, made.height).cpu().numpy().view(np.uint32), events.shape[0])
        assert msg is None, msg
        swapped = dict(tabs)
        swapped[chip] = (tabs[chip][0], _canonical_rows(made))
        assert frozenset(a.name for a, _ in machine) in RT.chip_clusters()
        assert MC.check_shard(machine, swapped, publics, PVM.program()) == ([], 0)
        dev = [(a, i, core_real.to_col_major(tabs[a.name][1].cuda()), core_real.to_col_major(tabs[a.name][0].cuda()) if tabs[a.name][0] is not None else None)
               for a, i in machine]
        commit, prep = api.JaggedProver(L, lsh, batch, 1).commit_multilinears([d[3] for d in dev if d[3] is not None])

        def prove(chips):
            ch = api.DuplexChallenger()
            ch.observe(commit)
            return api.prove_shard(chips, RT.to_monty_np(publics), prep, L, lsh, batch, ch, 1, 5, 4)
        assert prove([(a, i, made if a.name == chip else m, p) for a, i, m, p in dev]) == prove(dev)
        seen.append(kind)
    assert seen == ["secp256k1_add", "secp256k1_double"]
    g2 = SC.affine_add(SC.G, SC.G)
    g3 = SC.affine_add(SC.G, g2)
    gm = {int(r[0]): int(r[2]) & SC.M64 for r in ex.global_memory()}
    point = lambda off: tuple(sum(gm[0x78100000 + off + 32 * c + 8 * k] << (64 * k) for k in range(4)) for c in range(2))
    assert point(0) == g2 and point(64) == SC.affine_add(g3, g3)
