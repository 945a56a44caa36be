"""GPU (-m gpu): device trace generation for the RISC-V Global chip (sp1hip_tracegen_riscv_global) — from the
(message, is_receive, kind) events alone the device table equals the host trace of riscv_trace.py / septic.py word for word
(Poseidon2 columns, lifted curve points, offsets, range-check bytes, the running digest sum, the padding rows), and a shard proven
from the device-generated table equals the proof from the host table.

The sizes of tests/global_cases.py (one set of 32,800 distinct legal events, lifted once by septic.py on the device; every case a
prefix) reach what the two older tests do not: chunk edges, the chunk-sum and finalize kernels across a 256-lane workgroup, and both
regimes of global_scan_totals_kernel — slices of one chunk per lane up to 16,384 events, longer slices with fewer live lanes and a
short last slice above. Each case is checked twice: word for word against the host table, and by a route that does not pass through
septic.py's scan — every constraint of the Global AIR on every row of the DEVICE table, the chain initial_digest[i] ==
cumulative_sum[i - 1] from the start point, and for small n the last sum against one addition after the other in Python integers
(tests/septic_model.py). The failed path (no point within 256 offsets) needs a Poseidon2 preimage and is not reached."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_cases as G  # noqa: E402
import machine_check as MC  # noqa: E402
import septic_model as M  # noqa: E402


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _events(main, n):
    """[n, 9] int32 events from the host trace's message / is_receive / kind columns."""
    L = R.chip("Global")[0].layout
    ev = torch.zeros((n, 9), dtype=torch.int64, device=main.device)
    ev[:, :8] = main[:n, L["message"]:L["message"] + 8]
    ev[:, 8] = main[:n, L["is_receive"]] | (main[:n, L["kind"]] << 8)
    return ev.to(torch.int32).contiguous()


@pytest.mark.parametrize("counts,K", [({"Add": 4, "LoadWord": 6, "StoreWord": 6, "UType": 8, "Ecall": 6}, 2),
                                      ({"Add": 40, "Addi": 40, "LoadByte": 60, "LoadDouble": 60, "StoreByte": 60, "StoreDouble": 60, "UType": 30, "Branch": 20}, 3)])
def test_device_global_trace_equals_the_host_trace(api, counts, K):
    import core_real
    machine, tabs, _ = RT.generate(counts, K=K, seed=17, device="cuda")
    main = tabs["Global"][1]
    n = int((main[:, R.chip("Global")[0].layout["is_real"]] == 1).sum())
    assert 0 < n <= main.shape[0] and main.shape[0] > n                  # padding rows are part of the comparison
    got = api.tracegen_riscv_global(_events(main, n), main.shape[0])
    want = core_real.to_col_major(main)
    assert got.height == want.height and got.width == want.width
    g, w = got.words.view(got.width, got.height), want.words.view(want.width, want.height)
    bad = (g != w).nonzero()
    assert bad.numel() == 0, ("first mismatch (column, row):", bad[0].tolist())


def test_shard_proof_from_the_device_generated_global_table(api):
    import core_real
    counts = {"Add": 4, "Addi": 6, "LoadWord": 6, "StoreWord": 6, "UType": 8, "Branch": 4}
    machine, tabs, publics = RT.generate(counts, K=2, seed=19, device="cuda")
    dev = [(a, i, core_real.to_col_major(tabs[a.name][1]), core_real.to_col_major(tabs[a.name][0]) if tabs[a.name][0] is not None else None)
           for a, i in machine]
    L, lsh, batch = 17, 12, 8
    commit, prep = api.JaggedProver(L, lsh, batch, 1).commit_multilinears([d[3] for d in dev if d[3] is not None])

    def prove(chips):
        ch = api.DuplexChallenger()
        ch.observe(commit)
        return api.prove_shard(chips, RT.to_monty_np(publics), prep, L, lsh, batch, ch, 1, 5, 4)
    want = prove(dev)
    main = tabs["Global"][1]
    n = int((main[:, R.chip("Global")[0].layout["is_real"]] == 1).sum())
    table = api.tracegen_riscv_global(_events(main, n), main.shape[0])
    dev2 = [(a, i, table if a.name == "Global" else m, p) for a, i, m, p in dev]
    assert prove(dev2) == want


# ---------------------------------------------------------------------------------------------- the sizes of tests/global_cases.py
@pytest.fixture(scope="module")
def full(api):
    """(the 32,800 events on the device as int32 [n, 9], the host trace of all of them: lifted and summed ONCE)"""
    ev = G.events()
    d_ev = torch.tensor(ev.astype(np.int32), device="cuda").contiguous()
    return d_ev, G.Reference(ev, "cuda")


def _canonical_rows(words, height):
    """device table words [241 * height] -> canonical uint64 numpy [height, 241]"""
    t = words.view(G.WIDTH, height).to(torch.int64) & 0xFFFFFFFF
    return (t * G.R_INV % G.P).t().contiguous().cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("n,height", G.SIZES, ids=["%d-%d" % s for s in G.SIZES])
def test_device_global_table_at_the_scan_and_workgroup_edges(api, full, n, height):
    d_ev, ref = full
    got = api.tracegen_riscv_global(d_ev[:n], height)
    assert got.height == height and got.width == G.WIDTH
    # (a) word for word the host table, padding rows included
    bad = (got.words.view(G.WIDTH, height) != ref.words(n, height)).nonzero()
    assert bad.numel() == 0, ("first mismatch (column, row):", bad[0].tolist(), "of", bad.shape[0])
    # (b) without septic.py's scan: the AIR's constraints on every row of the device table ...
    air, L = R.chip("Global")[0], R.chip("Global")[0].layout
    main = _canonical_rows(got.words, height)
    publics = np.zeros(1024, np.uint64)
    for lo in range(0, height, 4096):
        vals = MC.constraint_values(air, None, main[lo:lo + 4096], publics)
        assert vals.shape[1] == air.num_constraints
        nz = np.argwhere(vals != 0)
        assert nz.size == 0, ("constraint does not vanish (row, constraint):", [lo + int(nz[0][0]), int(nz[0][1])], len(nz))
    # ... and the chain of running sums from the start point
    ix, iy, cx, cy = (L["accumulation." + k] for k in ("initial_digest_x", "initial_digest_y", "cumulative_sum_x", "cumulative_sum_y"))
    if n:
        assert main[0, ix:ix + 7].tolist() == M.START[0] and main[0, iy:iy + 7].tolist() == M.START[1]
        assert (main[1:n, ix:ix + 7] == main[:n - 1, cx:cx + 7]).all() and (main[1:n, iy:iy + 7] == main[:n - 1, cy:cy + 7]).all()
        assert (main[:n, L["is_real"]] == 1).all() and (main[:n, L["index"]] == np.arange(n)).all()
    assert (main[n:, L["is_real"]] == 0).all()
    if 0 < n <= 300:
        xc, yc = L["interaction.x_coordinate"], L["interaction.y_coordinate"]
        pts = [(main[i, xc:xc + 7].tolist(), main[i, yc:yc + 7].tolist()) for i in range(n)]
        last = M.sequential_sum(pts)[-1]
        assert (main[n - 1, cx:cx + 7].tolist(), main[n - 1, cy:cy + 7].tolist()) == last


def _raw_call(api, out, height, events, n):
    from sp1_amd import _lib
    import ctypes as C
    return _lib.load().sp1hip_tracegen_riscv_global(C.c_void_p(out.data_ptr()), int(height), C.c_void_p(events.data_ptr()) if events is not None else None,
                                                    int(n), C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_more_events_than_rows_is_refused_and_height_zero_succeeds(api, full):
    d_ev, _ = full
    sentinel = 0x5A5A5A5A
    out = torch.full((G.WIDTH * 32,), sentinel, dtype=torch.int32, device="cuda")
    assert _raw_call(api, out, 16, d_ev[:17], 17) != 0                     # n_events > height
    torch.cuda.synchronize()
    assert bool((out == sentinel).all()), "a refused call wrote to the table"
    assert _raw_call(api, out, 0, None, 0) == 0                            # an empty table
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())


def test_calls_of_different_sizes_on_one_stream_reuse_the_arena(api, full):
    d_ev, ref = full
    for n, height in ((4097, 4128), (17, 32), (4097, 4128), (0, 16), (1, 16)):
        got = api.tracegen_riscv_global(d_ev[:n], height)
        assert bool((got.words.view(G.WIDTH, height) == ref.words(n, height)).all()), (n, height)
