"""CPU: the rows of the four SHA-256 precompile chips and the quad segment form of the MemoryLocal records, as the device kernels
compute them, run on the host. tests/native/sha_rows (built by __graft_entry__.build()) includes sp1_amd/csrc/tg_sha256_rows.hpp and
tg_riscv_memglobal_rows.hpp unchanged; its `host` form runs the same row functions the kernels of tracegen_sha256.hip call, in a
plain loop, and never opens a GPU.

* the generator's records (tests/sha_cases.py, Python integers) pass the host builders' own assertions, and reach what they are
  meant to: both values of next_clk.is_overflow inside one call, the top address limbs, all three ways a previous timestamp stands
  to its access, upper halves of memory words;
* ShaCompress's padding rule, restated, equals the host builder's padding rows at the host builder's height;
* every word of the four tables equals the host builders' (sha_extend_shard_from / sha_compress_shard_from) at every shape of
  sha_cases.SHAPES, padding rows included — the restated padding behind the host builder's own height;
* the program's widths and column offsets equal R.chip(name)[0].main_width / .layout;
* the two descriptors' MemoryLocal records are the ones the host shard's MemoryLocal rows stand for, in its order, and through the
  pinned MemoryLocal and SyscallPrecompile row functions they give the host shard's tables and Global events; a quad segment that
  reads behind the record is refused;
* the same on the events of the sha2 guest (bytes(range(200)), 8000 cycles per shard);
* ShaExtend's and ShaCompress's constraints vanish on every row of the host-form tables.
Everything is bit-exact; there are no tolerances."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import machine_check as MC  # noqa: E402
import memory_global_cases as G  # noqa: E402
import riscv_core_row_cases as K  # noqa: E402
import sha_cases as S  # noqa: E402

from sp1_amd.machines import riscv as R  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from sp1_amd.machines import riscv_trace as RT  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    assert os.path.exists(S.EXE), "tests/native/sha_rows is not built: run __graft_entry__.build()"


def test_the_generated_events_pass_the_host_builders_assertions_and_reach_their_cases():
    """host_chip_tables runs sha_*_shard_from, which asserts that w[i] is the extension and the digest the compression."""
    ext = S.host_chip_tables("sha_extend", 11)["ShaExtend"].numpy()
    lay = R.chip("ShaExtend")[0].layout
    over = ext[:48, lay["next_clk.is_overflow"]]
    assert over[:22].sum() == 0 and over[22:].all()                                   # event 0 crosses 2^24 at r = 22
    assert (ext[48:96, lay["w_ptr"] + 1:lay["w_ptr"] + 3] == 0xFFFF).all()            # event 1: both upper address limbs full
    assert len(set(ext[96:144, lay["w_i_ptr.value"] + 1].tolist())) == 2              # event 2: a carry into the second limb inside the call
    for name in ("w_i_minus_15", "w_i_minus_2", "w_i_minus_16", "w_i_minus_7", "w_i"):
        at = lay[name + ".prev_value"]
        live = ext[:48 * 11]
        assert set(live[:, at + 6].tolist()) == {0, 1}, name                          # compare_low both ways
        assert ((live[:, at + 7] == 0) & (live[:, at + 8] == 0) & (live[:, at + 6] == 1)).any(), name     # a difference of 0
    assert ext[:48 * 11, lay["w_i.prev_value"] + 2:lay["w_i.prev_value"] + 4].any()   # upper halves in the words overwritten
    assert ext[:48 * 11, lay["w_i_minus_15.prev_value"] + 2:lay["w_i_minus_15.prev_value"] + 4].any()
    cmp = S.host_chip_tables("sha_compress", 7)["ShaCompress"].numpy()
    lay = R.chip("ShaCompress")[0].layout
    at = lay["mem.prev_value"]
    live = cmp[:80 * 7]
    assert set(live[:, at + 6].tolist()) == {0, 1} and live[:, at + 2:at + 4].any()
    assert ((live[:, at + 7] == 0) & (live[:, at + 8] == 0) & (live[:, at + 6] == 1)).any()
    assert (cmp[80:160, lay["h_ptr"] + 1:lay["h_ptr"] + 3] == 0xFFFF).all()
    assert len(set(cmp[240:320, lay["clk_high"]].tolist())) == 1 and cmp[240, lay["clk_low"]] == (1 << 24) - 7    # event 3: the window's last slot
    words = np.concatenate([S.events(k, 7).view(np.uint64)[:, 3:].reshape(-1) for k in S.KINDS]) & np.uint64(S.M32)
    assert set(S.EDGE) <= set(int(v) for v in words)


@pytest.mark.parametrize("n", [1, 3, 7])
def test_the_restated_padding_is_the_host_builders(n):
    host = S.host_chip_tables("sha_compress", n)["ShaCompress"].numpy()
    assert host.shape[0] == RT.pad32(80 * n) > 80 * n
    assert np.array_equal(host[80 * n:], S.compress_padding(80 * n, host.shape[0]))
    assert host[80 * n:].any()                                                        # not zero rows


@pytest.mark.parametrize("chip,n,height", S.CHIP_SHAPES)
def test_every_word_equals_the_host_builder(chip, n, height, tmp_path):
    want = S.montgomery_col_major(S.expected_table(chip, n, height))
    got = S.run_rows("host", chip, S.events(S.KIND_OF[chip], n), height, tmp_path)
    msg = S.first_difference(chip, want, got, S.ROWS_PER_CALL[chip] * n)
    assert msg is None, msg


def test_rows_that_do_not_fit_are_refused(tmp_path):
    for chip, n, height in (("ShaExtend", 2, 64), ("ShaCompress", 1, 64), ("ShaExtendControl", 33, 32)):
        with pytest.raises(subprocess.CalledProcessError):
            S.run_rows("host", chip, S.events(S.KIND_OF[chip], n), height, tmp_path)


def test_widths_and_column_constants_equal_the_transcribed_chips():
    text = subprocess.run([S.EXE, "host", "layout"], check=True, capture_output=True, timeout=60).stdout.decode()
    seen = {}
    for line in text.splitlines():
        chip, key, col = line.split()
        air = R.chip(chip)[0]
        assert int(col) == (air.main_width if key == "width" else air.layout[key]), line
        seen.setdefault(chip, set()).add(key)
    assert set(seen) == set(S.ROWS_PER_CALL)
    for chip in ("ShaExtendControl", "ShaCompressControl"):
        assert seen[chip] == set(R.chip(chip)[0].layout) | {"width"}, chip
    # every column group of the wide chips is among them
    for chip in ("ShaExtend", "ShaCompress"):
        groups = {k.split(".")[0] for k in R.chip(chip)[0].layout}
        assert groups == {k.split(".")[0] for k in seen[chip]} - {"width"}, chip


def _closing_tables_equal_the_host_shard(kind, ev, shard, tmp_path):
    """The records of the kind's segments, SyscallPrecompile and their Global events against the host shard of the same events."""
    _, tables, _, gev = shard
    n, per_call = len(ev), sum(s[1] for s in S.SEGMENTS[kind])
    sp, ml = tables["SyscallPrecompile"][1], tables["MemoryLocal"][1]
    assert ml.shape[0] == RT.pad32(per_call * n) and gev.shape[0] == (2 * per_call + 1) * n
    want_events = G.reduce_global_events(gev)
    records = S.run_records(ev, S.SEGMENTS[kind], tmp_path)
    assert records.shape == (per_call * n, 5)
    want = G.local_records_of(ml[:per_call * n])
    assert np.array_equal(records, want), np.argwhere(records != want)[:4]
    table = K.run_rows("MemoryLocal", records, int(ml.shape[0]), tmp_path)
    msg = K.first_difference("MemoryLocal", G.montgomery_col_major(ml), table, per_call * n)
    assert msg is None, msg
    assert np.array_equal(K.run_global(records, tmp_path), want_events[:2 * per_call * n])
    args = (S.WORDS[kind],) + S.SYSCALL[kind]
    got = G.run_rows("SyscallPrecompile", ev, int(sp.shape[0]), tmp_path, args)
    msg = G.first_difference("SyscallPrecompile", G.montgomery_col_major(sp), got, n)
    assert msg is None, msg
    assert np.array_equal(G.run_global("SyscallPrecompile", ev, tmp_path, args), want_events[2 * per_call * n:])


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("n", S.SHARD_CALLS)
def test_local_records_and_closing_chips_equal_the_host_shard(kind, n, tmp_path):
    ev = S.shard_events(kind, n)
    _closing_tables_equal_the_host_shard(kind, ev, S.host_shard(kind, ev, key=(kind, n)), tmp_path)


def test_the_descriptors_are_the_ones_the_api_uses():
    from sp1_amd import api
    assert S.QUAD == api.PRECOMPILE_QUAD_WORDS and set(api.SHA_DESCRIPTORS) == set(S.KINDS) == set(X.DEVICE_SHA_KINDS)
    for kind in S.KINDS:
        assert api.SHA_DESCRIPTORS[kind] == (S.WORDS[kind],) + S.SYSCALL[kind] + (S.SEGMENTS[kind],), kind
        chip, control, rows, touched = X.PRECOMPILES[kind]
        assert (chip, control) == S.CHIPS[kind] and rows == S.ROWS_PER_CALL[chip] and touched == sum(s[1] for s in S.SEGMENTS[kind])


def test_a_quad_segment_that_reads_behind_the_record_is_refused(tmp_path):
    ev = S.events("sha_extend", 1)
    assert S.run_records(ev, ((1, 64, 530, S.QUAD, 0),), tmp_path) is not None
    for bad in ((1, 64, 531, S.QUAD, 0), (1, 65, 530, S.QUAD, 0), (1, 197, 0, S.QUAD, 0), (786, 1, 0, S.QUAD, 0)):
        assert S.run_records(ev, (bad,), tmp_path, check=False) is None, bad


@pytest.fixture(scope="module")
def sha2_records():
    """The sha_extend and sha_compress records of the sha2 guest's run, and the host shard of each."""
    import test_tracegen_memglobal_abi as T
    guest, max_cycles = T.RUNS["sha2"]
    ex, out = guest(), {}
    for rec in X.run_records(ex, max_cycles):
        if rec.kind in S.KINDS:
            out[rec.kind] = (np.ascontiguousarray(rec.events), X.host_shard(ex, rec))
    assert set(out) == set(S.KINDS)
    return out


@pytest.mark.parametrize("kind", S.KINDS)
def test_the_sha2_guests_events_give_the_host_shards_tables(kind, sha2_records, tmp_path):
    ev, shard = sha2_records[kind]
    assert ev.shape[1] == S.WORDS[kind] and len(ev) >= 1
    for chip in S.CHIPS[kind]:
        main = shard[1][chip][1]
        got = S.run_rows("host", chip, ev, int(main.shape[0]), tmp_path)
        msg = S.first_difference(chip, G.montgomery_col_major(main), got, S.ROWS_PER_CALL[chip] * len(ev))
        assert msg is None, msg
    _closing_tables_equal_the_host_shard(kind, ev, shard, tmp_path)


@pytest.mark.parametrize("kind", S.KINDS)
def test_constraints_vanish_on_every_table_of_the_one_call_shard(kind, tmp_path):
    """The shard the GPU test proves: the two chips' host-form tables and the host shard's closing tables."""
    ev = S.shard_events(kind, 1)
    _, tables, publics, _ = S.host_shard(kind, ev, key=(kind, 1))
    for name in S.CHIPS[kind] + ("SyscallPrecompile", "MemoryLocal"):
        air = R.chip(name)[0]
        main = tables[name][1].numpy().astype(np.uint64)
        if name in S.CHIPS[kind]:
            main = MC.from_monty(S.run_rows("host", name, ev, int(main.shape[0]), tmp_path).T)
        cv = MC.constraint_values(air, None, main, publics.numpy().astype(np.uint64))
        assert not cv.any(), (name, sorted(set(np.argwhere(cv != 0)[:, 1]))[:8])


@pytest.mark.parametrize("kind", S.KINDS)
def test_constraints_vanish_on_the_host_form_tables(kind, sha2_records, tmp_path):
    """On the guest's events and on the generator's with clean upper halves (the chips' constraints want the words read to be
    32-bit; the words SHA_EXTEND overwrites keep their upper halves) — at the host builder's height and one beyond it."""
    chip = S.CHIPS[kind][0]
    air = R.chip(chip)[0]
    publics = np.zeros(X.PV_WORDS, dtype=np.uint64)                                   # the chips read no public value
    rows = S.ROWS_PER_CALL[chip]
    for ev in (sha2_records[kind][0], S.events(kind, 5, upper=False)):
        for height in (RT.pad32(rows * len(ev)), RT.pad32(rows * len(ev)) + 96):
            main = MC.from_monty(S.run_rows("host", chip, ev, height, tmp_path).T)
            cv = MC.constraint_values(air, None, main, publics)
            assert cv.shape == (height, air.num_constraints) and not cv.any(), (len(ev), height, sorted(set(np.argwhere(cv != 0)[:, 1]))[:8])
