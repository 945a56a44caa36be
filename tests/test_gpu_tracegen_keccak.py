"""GPU (-m gpu): device trace generation for the Keccak precompile chips (sp1hip_tracegen_riscv_keccak: KeccakPermute, 24 rows of
2,640 columns per call; sp1hip_tracegen_riscv_keccak_control: KeccakPermuteControl, 634 columns) against the host fillers of the
same events (riscv_more_trace.keccak_permute_table / precompile_shard_from): every word of every column, padding rows included,
bit for bit. Shapes: padding only, a partial trailing chunk, no padding, an event across a workgroup boundary, several
workgroups. States: zero, ones, single bits at the limb edges of three lanes (one of them the lane rotated by 62), the two outer
bits of every lane, random. Clocks across and next to a 2^24 boundary, addresses with upper limbs. The permutation itself is
pinned by hashlib's SHA3-256, the two tables by each other (row 23's sent state = the controller's final_value), and a shard
proof made from the device tables of a real guest's Keccak shard equals the proof from the host tables."""
import hashlib
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench"))
from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_more_trace as MT  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

I64 = torch.int64
NAMES = ("KeccakPermute", "KeccakPermuteControl")
SHAPES = [(0, 32), (1, 32), (4, 96), (11, 288), (43, 1056)]          # (events, KeccakPermute rows)
START = {0: 0, 1: 1, 4: 13, 11: 0, 43: 0}                            # where in the state list a shape's events begin
CLK0 = (5 << 24) + 1001                                              # clk_high = 5


def _s64(v):
    return v - (1 << 64) if v >> 63 else v


def _states():
    """43 states [43, 25] (lane x + 5 y): zero, ones, one bit at 0 / 15 / 16 / 63 of lane (0,0), of lane (4,4), of the lane rotated
    by 62 (x = 2, y = 0), 0x8000...0001 everywhere, then random ones."""
    assert MT.M.KECCAK_R[2][0] == 62
    out = [[0] * 25, [-1] * 25]
    for lane in (0, 24, 2):
        for bit in (0, 15, 16, 63):
            st = [0] * 25
            st[lane] = _s64(1 << bit)
            out.append(st)
    out.append([_s64((1 << 63) | 1)] * 25)
    gen = torch.Generator()
    gen.manual_seed(20)
    rnd = torch.randint(RT.MIN64, (1 << 63) - 1, (43 - len(out), 25), generator=gen, dtype=I64)
    return torch.cat([torch.tensor(out, dtype=I64), rnd])


def _calls(n):
    """n system calls: (clk [n], addr [n], pre [n, 25], t_prev [n, 25]) on the device."""
    idx = (START[n] + torch.arange(n)) % 43
    pre = _states()[idx]
    gen = torch.Generator()
    gen.manual_seed(n)
    clk = CLK0 + 320 * torch.arange(n, dtype=I64)
    addr = 0x20_0000 + 256 * torch.randperm(4 * n + 4, generator=gen)[:n].to(I64)
    t_prev = torch.randint(1, CLK0 - 8, (n, 25), generator=gen, dtype=I64)       # both sides of the 5 << 24 boundary
    if n:
        t_prev[0, 0] = clk[0] - 1                                                # the access just before
        t_prev[0, 1] = (5 << 24) - 1                                             # the last tick of the window before clk's
        t_prev[0, 2] = 5 << 24                                                   # the first tick of clk's window
        t_prev[0, 3] = 1
    if n >= 4:
        clk[n - 1] = (6 << 24) + 1                                               # a call on the first cycle of a window
        t_prev[n - 1, 0], t_prev[n - 1, 1], t_prev[n - 1, 2] = 6 << 24, (6 << 24) - 1, 1
        addr[1] = 0xFFFF_FFFF_0000                                               # both upper limbs full: top_two_limb_max is zero
        addr[2] = 0x0001_0002_FFF8                                               # addr + 8 carries into the second limb
        addr[3] = 0x1234_0000_0100
    return [t.cuda() for t in (clk, addr, pre, t_prev)]


def _events(clk, addr, pre, t_prev, post):
    n = clk.shape[0]
    ev = torch.zeros((n, 77), dtype=I64, device=clk.device)
    ev[:, 0], ev[:, 1] = clk, addr
    ev[:, 2:52:2], ev[:, 3:52:2], ev[:, 52:] = t_prev, pre, post
    return ev


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


_CASES = {}


def _case(api, n, height):
    """Host and device tables of a shape, made once: {name: (want [width, height], got [width, height])}, the events, post."""
    if n in _CASES:
        return _CASES[n]
    import core_real
    clk, addr, pre, t_prev = _calls(n)
    dev = torch.device("cuda")
    if n:
        _, tabs, _, _ = MT.precompile_shard_from(clk, addr, pre, t_prev, dev)
        host = {name: tabs[name][1] for name in NAMES}
        post = MT.keccak_round_tensors(pre)[1]
    else:                                   # no host shard without a call: the zero state's rounds, q mod 24, nothing else set
        zero = MT.keccak_permute_table(torch.zeros(1, dtype=I64, device=dev), torch.zeros(1, dtype=I64, device=dev),
                                       torch.zeros((1, 25), dtype=I64, device=dev), dev)[0].main[:24].clone()
        zero[:, R.chip(NAMES[0])[0].layout["clk_high"]:] = 0
        host = {NAMES[0]: zero[torch.arange(height, device=dev) % 24], NAMES[1]: torch.zeros((32, 634), dtype=I64, device=dev)}
        post = torch.zeros((0, 25), dtype=I64, device=dev)
    assert host[NAMES[0]].shape[0] == height and host[NAMES[1]].shape[0] == RT.pad32(n) or n == 0
    ev = _events(clk, addr, pre, t_prev, post)
    got = MT.keccak_device_tables(ev, [host[name].shape[0] for name in NAMES])
    out = {}
    for name, g in zip(NAMES, got):
        w = core_real.to_col_major(host[name])
        assert (g.width, g.height) == (w.width, w.height) == (R.chip(name)[0].main_width, host[name].shape[0])
        out[name] = (w.words.view(w.width, w.height), g.words.view(g.width, g.height), g)
    _CASES[n] = (out, ev, post)
    return _CASES[n]


def _group(name, col):
    lay = R.chip(name)[0].layout
    at = max(c for c in lay.values() if c <= col)
    return sorted(k for k, c in lay.items() if c == at)[0]


def _assert_equal(name, want, got, n):
    bad = (got != want).nonzero()
    if bad.numel():
        col, row = bad[0].tolist()
        rule = "event %d round %d" % (row // 24, row % 24) if name == NAMES[0] else "event %d" % row
        pytest.fail("%s with %d events: %d words differ; first at column %d (group %s), row %d (%s): got %#x, want %#x"
                    % (name, n, bad.shape[0], col, _group(name, col), row, rule, int(got[col, row]) & 0xFFFFFFFF, int(want[col, row]) & 0xFFFFFFFF))


def test_widths(api):
    assert api._L().sp1hip_tracegen_riscv_keccak_width() == R.chip(NAMES[0])[0].main_width
    assert api._L().sp1hip_tracegen_riscv_keccak_control_width() == R.chip(NAMES[1])[0].main_width


@pytest.mark.parametrize("n,height", SHAPES)
def test_permute_table_equals_the_host_filler(api, n, height):
    want, got, _ = _case(api, n, height)[0][NAMES[0]]
    _assert_equal(NAMES[0], want, got, n)


@pytest.mark.parametrize("n,height", SHAPES)
def test_control_table_equals_the_host_filler(api, n, height):
    want, got, _ = _case(api, n, height)[0][NAMES[1]]
    _assert_equal(NAMES[1], want, got, n)


def _canonical(words):
    """Montgomery int32 words -> canonical int64."""
    return (words.to(I64) & 0xFFFFFFFF) * pow(1 << 32, -1, RT.P) % RT.P


def _sent_state(table, rows):
    """The state the KeccakPermute rows `rows` send on: a_prime_prime_prime_0_0_limbs at (0, 0), a_prime_prime elsewhere; [len, 25]
    lanes as unsigned python ints."""
    lay = R.chip(NAMES[0])[0].layout
    app = _canonical(table[lay["keccak.a_prime_prime.0.0"]:lay["keccak.a_prime_prime.0.0"] + 100][:, rows]).t().reshape(-1, 25, 4)
    a0 = lay["keccak.a_prime_prime_prime_0_0_limbs"]
    app[:, 0] = _canonical(table[a0:a0 + 4][:, rows]).t()
    return [[sum(int(l) << (16 * k) for k, l in enumerate(lane)) for lane in st] for st in app.tolist()]


@pytest.mark.parametrize("n,height", [s for s in SHAPES if s[0]])
def test_row_23_sends_the_words_the_controller_holds(api, n, height):
    tabs, ev, post = _case(api, n, height)
    sent = _sent_state(tabs[NAMES[0]][1], 24 * torch.arange(n, device="cuda") + 23)
    written = [[int(v) & ((1 << 64) - 1) for v in row] for row in ev[:, 52:].tolist()]
    assert sent == written
    lay = R.chip(NAMES[1])[0].layout
    fv = _canonical(tabs[NAMES[1]][1][lay["final_value.0"]:lay["final_value.0"] + 100][:, :n]).t().reshape(n, 25, 4).tolist()
    assert [[sum(int(l) << (16 * k) for k, l in enumerate(lane)) for lane in st] for st in fv] == written


def test_the_permutation_is_sha3_256s(api):
    msg = b"device trace generation"
    block = bytearray(200)
    block[:len(msg)] = msg
    block[len(msg)] ^= 0x06                                  # SHA-3's domain bits and the first pad bit
    block[135] ^= 0x80                                       # rate 136 bytes: the last pad bit
    pre = torch.tensor([[_s64(int.from_bytes(block[8 * i:8 * i + 8], "little")) for i in range(25)]], dtype=I64, device="cuda")
    ev = _events(torch.tensor([CLK0], device="cuda"), torch.tensor([0x20_0000], device="cuda"), pre, torch.ones((1, 25), dtype=I64, device="cuda"),
                 torch.zeros((1, 25), dtype=I64, device="cuda"))
    table = api.tracegen_riscv_keccak(ev, 32)
    out = _sent_state(table.words.view(table.width, table.height), torch.tensor([23], device="cuda"))[0]
    assert b"".join(v.to_bytes(8, "little") for v in out[:4]) == hashlib.sha3_256(msg).digest()


def test_argument_checks(api):
    ev = torch.zeros((2, 77), dtype=I64, device="cuda")
    with pytest.raises(api._lib.Sp1HipError):
        api.tracegen_riscv_keccak(ev, 32)                    # 48 rows do not fit
    with pytest.raises(api._lib.Sp1HipError):
        api.tracegen_riscv_keccak_control(ev, 1)
    assert api.tracegen_riscv_keccak(ev[:0], 0).words.numel() == 0


def test_the_keccak_shard_of_a_real_guest(api):
    """keccak.elf on 300 zero bytes: the Keccak shard's two device tables equal the host ones (the written words come from the
    executor here, not from the filler), and a shard proof made with them is the proof from the host tables, byte for byte."""
    import core_real
    ex = X.Executor(X.guest_file("keccak.elf"), stdin=[bytes(300)])
    kev = [rec for rec in X.run_records(ex, 6000, core_limit=0) if rec.kind == "keccak"]
    if not kev:
        pytest.fail("the guest made no Keccak shard")
    machine, tabs, publics, gev = X.host_shard(ex, kev[0], "cuda")
    kev = [rec.events for rec in kev]
    assert len(kev) == 1 and kev[0].shape[0] > 0 and kev[0].shape[1] == 77
    made = dict(zip(NAMES, MT.keccak_device_tables(kev[0], [tabs[name][1].shape[0] for name in NAMES])))
    dev = [(a, i, core_real.to_col_major(tabs[a.name][1]), core_real.to_col_major(tabs[a.name][0]) if tabs[a.name][0] is not None else None)
           for a, i in machine]
    for a, _, m, _ in dev:
        if a.name in made:
            g = made[a.name]
            _assert_equal(a.name, m.words.view(m.width, m.height), g.words.view(g.width, g.height), kev[0].shape[0])
    L, lsh, batch = 17, 12, 8
    commit, prep = api.JaggedProver(L, lsh, batch, 1).commit_multilinears([d[3] for d in dev if d[3] is not None])

    def prove(chips):
        ch = api.DuplexChallenger()
        ch.observe(commit)
        return api.prove_shard(chips, RT.to_monty_np(publics), prep, L, lsh, batch, ch, 1, 5, 4)
    want = prove(dev)
    assert prove([(a, i, made.get(a.name, m), p) for a, i, m, p in dev]) == want
