"""CPU: the byte-lookup count of sp1_amd/csrc/tg_lookup_counts.hpp in its host form (tests/native/lookup_counts host: the same
__host__ __device__ row function the kernel runs, in a serial loop; no GPU, no library).

On the generated shard of tests/lookup_count_cases.py every chip counted alone over its padded table equals a torch tally of its
byte sends, and all chips together with the public values' row equal the host tracer's Byte and Range main tables, whole. Synthetic
one-send chips at heights 1, 63, 64, 65 and 257: every row on one cell, every row on its own, a multiplicity that is a sum of two
flags, multiplicity 0 on rows that hold rubbish, rows that share a cell with different multiplicities, every opcode at its edges, a variable opcode, weights and constants, preprocessed
columns. Each rule a message must keep is broken in one row: the status names that send and row and no count moves for it. Malformed
descriptions are refused. Everything is integers: whole arrays, exact equality."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lookup_count_cases as LC  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _program():
    assert os.path.exists(LC.EXE), "tests/native/lookup_counts is not built: run __graft_entry__.build()"


def _run_rows(it, rows, tmp_path, prep=None):
    return LC.run("host", it.to_array(), LC.col_major(np.array(rows, dtype=np.int64)), prep, tmp_path)


@pytest.fixture(scope="module")
def per_chip(tmp_path_factory):
    """{chip: (byte, range, status)} of the host form over every sending chip's padded table, once."""
    machine, tabs, _ = LC.shard()
    out = {}
    assert list(LC.SENDERS) == [n for n in sorted(tabs) if n not in ("Byte", "Range") and tabs[n][1].shape[0]]
    for name in LC.SENDERS:
        prep, main = tabs[name]
        out[name] = LC.run("host", machine[name][1].to_array(), LC.col_major(main), LC.col_major(prep) if prep is not None else None,
                           tmp_path_factory.mktemp(name))
    return out


def test_each_chip_equals_a_torch_tally(per_chip):
    machine, tabs, _ = LC.shard()
    total = 0
    for name, (byte, rng, status) in per_chip.items():
        prep, main = tabs[name]
        want_byte, want_range, n_bad = LC.torch_tally(machine[name][1], main, prep)
        assert n_bad == 0, name
        assert np.array_equal(byte, want_byte) and np.array_equal(rng, want_range), name
        assert not status.any(), (name, status)
        total += int(byte.sum()) + int(rng.sum())
    assert total > 6000                                        # the shard sends 6,759 messages with its public values


def test_all_chips_and_the_public_values_equal_the_tracers_tables(per_chip, tmp_path):
    _, tabs, _ = LC.shard()
    it, row = LC.public_values_row()
    byte, rng, status = LC.run("host", it.to_array(), LC.col_major(row), None, tmp_path)
    assert not status.any() and int(byte.sum()) + int(rng.sum()) == 56
    byte, rng = byte.astype(np.int64), rng.astype(np.int64)
    for b, r, _ in per_chip.values():
        byte += b
        rng += r
    assert np.array_equal(byte, tabs["Byte"][1].numpy().T)
    assert np.array_equal(rng, tabs["Range"][1].numpy()[:, 0])
    assert int(byte.sum()) + int(rng.sum()) == 6759
    assert int(byte.max()) == 1700 and int(rng.max()) == 794   # the skew the kernel is built for


@pytest.mark.parametrize("h", LC.HEIGHTS)
def test_synthetic_shapes(h, tmp_path):
    it = LC.message_chip()
    for name, rows in LC.table_cases(h).items():
        byte, rng, status = _run_rows(it, rows, tmp_path)
        want_byte, want_range, bad = LC.model(rows)
        assert not bad and not status.any(), name
        assert np.array_equal(byte, want_byte) and np.array_equal(rng, want_range), name
        if name == "one_cell":
            assert rng[256 + 5] == h and int(rng.sum()) == h and not byte.any()
        if name == "distinct_cells":
            assert (rng[65536:65536 + h] == 1).all() and int(rng.sum()) == h
        if name == "two_flags":
            assert int(byte.sum()) == 2 * h


def test_every_opcode_at_its_edges(tmp_path):
    rows = LC.edge_rows()
    byte, rng, status = _run_rows(LC.message_chip(), rows, tmp_path)
    want_byte, want_range, bad = LC.model(rows)
    assert not bad and not status.any()
    assert np.array_equal(byte, want_byte) and np.array_equal(rng, want_range)
    assert rng[1] == 1 and rng[131071] == 1 and rng[65536] == 1 and rng[3] == 1
    assert byte[5, 0x7F00] == 1 and byte[5, 0x8000] == 1 and byte[0, 0xFFFF] == 1 and byte[3, 0] == 1


def test_weights_constants_and_preprocessed_columns(tmp_path):
    inv_rows = [(1, 8 * i + 16, 16) for i in range(65)] + [(0, 5, 1)]          # (x - y) / 8 + 1 = i + 1; the last row sends nothing
    byte, rng, status = _run_rows(LC.weighted_chip(), inv_rows, tmp_path)
    want = np.zeros(LC.RANGE_CELLS, np.uint32)
    want[(1 << 13) + 1:(1 << 13) + 66] = 2
    assert np.array_equal(rng, want) and not byte.any() and not status.any()
    rows = LC.table_cases(65)["two_flags"]
    prep = LC.col_major(np.array([r[4:6] for r in rows], dtype=np.int64))
    main = [r[:4] + (0, 0) for r in rows]                                      # b and c come from the preprocessed table alone
    byte, rng, status = _run_rows(LC.message_chip(prep_columns=True), main, tmp_path, prep=prep)
    want_byte, want_range, _ = LC.model(rows)
    assert np.array_equal(byte, want_byte) and np.array_equal(rng, want_range) and not status.any()


@pytest.mark.parametrize("name", sorted(LC.BAD_ROWS))
def test_a_bad_message_is_named_and_moves_no_count(name, tmp_path):
    rows = LC.bad_table(name)
    byte, rng, status = _run_rows(LC.message_chip(), rows, tmp_path)
    want_byte, want_range, bad = LC.model(rows)
    assert [r for r, _ in bad] == [64]
    assert status[:4].tolist() == [1, 1, LC.SEND, 64], status
    assert np.array_equal(byte, want_byte) and np.array_equal(rng, want_range)
    assert int(byte.sum()) + int(rng.sum()) == 64


@pytest.mark.parametrize("name", sorted(LC.malformed()))
def test_malformed_descriptions_are_refused(name, tmp_path):
    words, main_width, prep_width = LC.malformed()[name]
    main = np.zeros((main_width, 32), np.uint32)
    with pytest.raises(LC.Rejected):
        LC.run("host", words, main, np.zeros((prep_width, 32), np.uint32) if prep_width else None, tmp_path)
