"""GPU: the device trace checker — api.check_constraints, api.check_interactions, riscv_exec.check_device_shard
(sp1_amd/csrc/trace_check.hip) — against tests/machine_check.py (numpy on the caller's programs, nothing of the library) on a host
copy of the same tables. Everything is integers: every field of every report, and the exact imbalance dictionary, equal.

No table is above 320 rows, except: the Byte (65,536 rows) and Range (131,072) lookup tables that every RISC-V shard holds, and
the two 100,000-row chips of `test_one_unbalanced_message_among_100000`, which is about a needle in that much hay.

* shards that should pass: the executed small shard of tests/lookup_count_cases.py (RT.generate, the 22 instruction kinds) staged
  from the host, and a hand-assembled program's shard made on the device by device_core_shard: zeros everywhere, "balanced";
* one corrupted cell of Bitwise, one of Global (on the device, one shard each): every field of the constraint report and the exact
  imbalance equal the host's on the corrupted copy;
* heights 0, 1, 63, 64, 65, 255, 256, 257 with failures on row 0 only, on the last row only, on one row in each of two workgroups
  (or the two ends of a shorter table), and on every row of a table with every constraint live (repair="all");
* KeccakPermute at 32 rows (the cut program), Bls12381DoubleAssign at 32 (the largest program, one wave per workgroup), DivRem at 300;
* stored words p and 2^32 - 1 are counted as non-canonical;
* buses: a bucket hit by every lane of a wave with different multiplicities, a multiplicity of p - 1, messages that cancel only
  across chips, one unbalanced message among 10^5, a `cap` below the records wanted, log_buckets = 4 against 22;
* bench/prove_program.py --elf <the carry program> --device-shard --check --verify: every shard "ok", the same proofs as without."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bench"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lookup_count_cases as LC  # noqa: E402
import machine_check as MC  # noqa: E402
import pyoracle as orc  # noqa: E402
import rv64_partition_cases as PC  # noqa: E402
import trace_check_cases as T  # noqa: E402
from kb_edges import EdgeSource  # noqa: E402
from sp1_amd import air as A  # noqa: E402
from sp1_amd.machines import public_values as PVM  # noqa: E402
from sp1_amd.machines import riscv_exec as X  # noqa: E402
from zc_arbitrary import arbitrary_chip, chip_air, publics_read, structurally_zero  # noqa: E402

P = T.P
HEIGHTS = (0, 1, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def api():
    from sp1_amd import api as a
    torch.cuda.set_device(0)
    return a


def _upload(api, monty_rows):
    """row-major Montgomery words [rows][width] -> ColMajor (None for None)."""
    if monty_rows is None:
        return None
    a = np.ascontiguousarray(monty_rows, dtype=np.uint32)
    if a.shape[0] == 0:
        return api.ColMajor(api.device_words(0), 0, a.shape[1])
    return api.ColMajor.from_row_major_host(a)


def _want(air, main, prep, publics):
    """The report machine_check implies for Montgomery tables (numpy)."""
    rows = main.shape[0]
    cv = T.host_values(air, main, prep, publics) if rows and air.num_constraints else np.zeros((rows, air.num_constraints), np.uint64)
    bad = np.nonzero(cv.any(axis=1))[0]
    first = int(bad[0]) if len(bad) else None
    return {"failing_rows": len(bad), "first_row": first, "fail_count": (cv != 0).sum(axis=0).astype(np.uint32),
            "first_constraints": [int(k) for k in np.nonzero(cv[first])[0][:64]] if len(bad) else [],
            "first_row_main": main[first] if len(bad) else None, "first_row_prep": prep[first] if len(bad) and prep is not None else None}


def _assert_report(got, want, what):
    assert got["failing_rows"] == want["failing_rows"] and got["first_row"] == want["first_row"], (what, got["failing_rows"], got["first_row"], want["failing_rows"], want["first_row"])
    assert np.array_equal(got["fail_count"], want["fail_count"]), what
    assert got["first_constraints"] == want["first_constraints"], what
    assert got["noncanonical"] == 0, what
    for k in ("first_row_main", "first_row_prep"):
        assert (got[k] is None) == (want[k] is None) and (want[k] is None or np.array_equal(got[k], want[k])), (what, k)


def _check(api, cases, publics):
    """cases: [(label, air, main, prep)] Montgomery row-major -> the reports of ONE call, each compared with the host's."""
    it = lambda air: A.InteractionProgram(air.name, air.main_width, air.prep_width)
    chips = [(air, it(air), _upload(api, main), _upload(api, prep)) for _, air, main, prep in cases]
    reports = api.check_constraints(chips, publics)
    assert [r["name"] for r in reports] == [c[1].name for c in cases]
    for (label, air, main, prep), got in zip(cases, reports):
        _assert_report(got, _want(air, main, prep, publics), label)
    return reports


# ---- shards that should pass ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def staged(api):
    """(machine [(air, it)], host tables {name: (prep, main)} canonical uint64, publics) of the executed small shard."""
    machine, tabs, publics = LC.shard()
    u64 = lambda t: None if t is None else t.numpy().astype(np.uint64)
    return [machine[n] for n in sorted(machine)], {n: (u64(p), u64(m)) for n, (p, m) in tabs.items()}, publics


def _stage(api, machine, host):
    return [(a, it, _upload(api, T.monty(host[a.name][1])), _upload(api, T.monty(host[a.name][0])) if host[a.name][0] is not None else None)
            for a, it in machine]


def test_a_satisfying_staged_shard_reports_nothing(api, staged):
    machine, host, publics = staged
    chips = _stage(api, machine, host)
    for r in api.check_constraints(chips, T.monty(publics.numpy())):
        assert r["failing_rows"] == 0 and r["first_row"] is None and r["noncanonical"] == 0 and not r["fail_count"].any() and r["first_constraints"] == [], r["name"]
    pv_air, pv_it = PVM.program()
    row = _upload(api, T.monty(publics.numpy()[None, :pv_it.main_width]))
    buses = api.check_interactions(chips + [(pv_air, pv_it, row, None)])
    assert buses["balanced"] and not buses["truncated"] and buses["imbalance"] == {} and buses["records_wanted"] == 0
    assert buses["nonzero_buckets"] == (0, 0) and buses["messages"] > 11000
    assert not api.check_interactions(chips)["balanced"]                   # without the public values' own messages a shard does not balance
    assert X.check_device_shard(machine, chips, publics) == ([], {})


def test_a_satisfying_device_made_shard_reports_nothing(api):
    import core_real
    ex, sh = PC.shard("core", False)
    prep = {n: core_real.to_col_major(t) for n, t in X.preprocessed_tables(PC.program("core")[0], "cuda").items()}
    machine, chips, publics, _ = X.device_core_shard(ex, sh, prep)
    assert X.check_device_shard(machine, chips, publics) == ([], {})
    words = T.monty(np.asarray(publics.cpu() if torch.is_tensor(publics) else publics, dtype=np.int64))
    assert all(r["failing_rows"] == 0 and r["noncanonical"] == 0 and not r["fail_count"].any() for r in api.check_constraints(chips, words))


# ---- corrupted cells ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["Bitwise", "Global"])
def test_one_corrupted_cell(api, staged, name):
    machine, host, publics = staged
    pv = publics.numpy().astype(np.uint64)
    air = dict((a.name, a) for a, _ in machine)[name]
    main = host[name][1]
    # the first cell of row 5 whose corruption breaks a constraint (numpy decides; the device is not asked)
    for col in range(air.main_width):
        bad = main.copy()
        bad[5, col] = (int(bad[5, col]) + 3) % P
        if MC.constraint_values(air, host[name][0], bad, pv).any():
            break
    else:
        raise AssertionError("no cell of row 5 matters")
    corrupted = dict(host)
    corrupted[name] = (host[name][0], bad)
    chips = _stage(api, machine, host)
    target = next(c for c in chips if c[0].name == name)[2]
    target.words.view(target.width, target.height)[col, 5] = int(np.asarray(T.monty([int(bad[5, col])])).view(np.int32)[0])      # on the device
    words = T.monty(pv)
    for got, (a, _) in zip(api.check_constraints(chips, words), machine):
        prep_h, main_h = corrupted[a.name]
        _assert_report(got, _want(a, T.monty(main_h), None if prep_h is None else T.monty(prep_h), words), a.name)
        assert (got["failing_rows"] != 0) == (a.name == name)
    pv_air, pv_it = PVM.program()
    want = MC.bus_imbalance([(it, corrupted[a.name][0], corrupted[a.name][1]) for a, it in machine] + [(pv_it, None, pv[None, :pv_it.main_width])])
    failing, imbalance = X.check_device_shard(machine, chips, publics)
    assert imbalance == want
    assert failing == [(name, [int(k) for k in np.nonzero(MC.constraint_values(air, host[name][0], bad, pv).any(axis=0))[0][:8]])]
    if name == "Global":
        assert want, "a Global row's message changed: its bus cannot balance"


# ---- edge heights and failure placement -------------------------------------------------------------------------------------------------
def _placed(name, h, rows_to_break, rng):
    """An all-zero table of `name` (which satisfies its constraints) with uniform words on the given rows."""
    air = chip_air(name)
    main = np.zeros((h, air.main_width), np.uint32)
    for r in rows_to_break:
        main[r] = orc.to_monty(rng.integers(0, P, size=air.main_width, dtype=np.uint64).astype(np.uint32))
    return air, main


@pytest.mark.parametrize("name", ["Add", "Mul"])
def test_edge_heights_and_failure_placement(api, name):
    rng = np.random.default_rng(17)
    publics = orc.random_felts((4,), 77)
    air = chip_air(name)
    assert not T.host_values(air, np.zeros((3, air.main_width), np.uint32), None, publics).any()
    cases = [("h0", air, np.zeros((0, air.main_width), np.uint32), None)]
    for h in HEIGHTS[1:]:
        two = sorted({3 % h, h - 1}) if h < 257 else [70, 256]              # 257 rows: the second and the last workgroup of 64, 128 or 256 lanes
        for label, rows in (("row0", [0]), ("last", [h - 1]), ("two", two), ("none", [])):
            cases.append(("%s-%d" % (label, h), air) + _placed(name, h, rows, rng)[1:] + (None,))
    reports = _check(api, cases, publics)
    by = {c[0]: r for c, r in zip(cases, reports)}
    assert by["h0"]["failing_rows"] == 0 and by["h0"]["first_row"] is None
    for h in HEIGHTS[1:]:
        assert by["row0-%d" % h]["first_row"] == 0 and by["last-%d" % h]["first_row"] == h - 1 and by["none-%d" % h]["failing_rows"] == 0
        assert by["row0-%d" % h]["failing_rows"] == by["last-%d" % h]["failing_rows"] == 1
    assert by["two-257"]["first_row"] == 70 and by["two-257"]["failing_rows"] == 2
    assert reports[1]["lanes"] in (64, 128, 256) and reports[1]["pieces"] == 1


@pytest.mark.parametrize("name", ["Add", "Mul"])
def test_every_row_fails_with_every_constraint_live(api, name):
    publics = orc.random_felts((4,), 77)
    cases = []
    for h in HEIGHTS[1:]:
        air, main, prep, _ = arbitrary_chip(name, h, np.random.default_rng(100 + h), repair="all")
        cases.append(("all-%d" % h, air, main, prep))
    reports = _check(api, cases, publics)
    for (label, air, main, _), r in zip(cases, reports):
        h = main.shape[0]
        assert r["failing_rows"] == h and r["first_row"] == 0, label
        if h >= 64:                                                        # every lane of every wave took the counter path
            live = [k for k in range(air.num_constraints) if k not in structurally_zero(air)]
            assert (r["fail_count"][live] > 0).all() and r["fail_count"].max() >= h - 2, label      # (a uniform word is 0 once in 2^31)


# ---- wide chips ---------------------------------------------------------------------------------------------------------------------------
def test_wide_chips(api):
    cases = []
    for name, rows, source in (("KeccakPermute", 32, EdgeSource(5)), ("Bls12381DoubleAssign", 32, np.random.default_rng(6)), ("DivRem", 300, EdgeSource(7))):
        air, main, prep = arbitrary_chip(name, rows, source)
        cases.append((name, air, main, prep))
    publics = orc.random_felts((publics_read([c[1] for c in cases]),), 77)
    keccak, bls, divrem = _check(api, cases, publics)
    assert keccak["pieces"] > 1 and keccak["lanes"] == 64 and keccak["failing_rows"] > 0
    assert bls["pieces"] == 1 and bls["lanes"] == 64 and bls["registers"] > 256 and bls["failing_rows"] == 32
    assert divrem["pieces"] == 1 and divrem["failing_rows"] > 250


# ---- non-canonical words ------------------------------------------------------------------------------------------------------------------
def test_noncanonical_words_are_counted(api):
    air = chip_air("Add")
    main = np.zeros((65, air.main_width), np.uint32)
    main[3, 2], main[64, air.main_width - 1] = P, 0xFFFFFFFF
    clean = np.zeros((65, air.main_width), np.uint32)
    clean[0, 0] = P - 1
    it = A.InteractionProgram("Add", air.main_width)
    got = api.check_constraints([(air, it, _upload(api, main), None), (air, it, _upload(api, clean), None)], orc.random_felts((4,), 77))
    assert got[0]["noncanonical"] == 2 and got[1]["noncanonical"] == 0


# ---- buses ------------------------------------------------------------------------------------------------------------------------------
V = A.VCol


def _bus_chip(name, sends=(), receives=(), width=2):
    """width-2 chips [m, v]: a message is (kind, [v or a constant]) with multiplicity column 0."""
    it = A.InteractionProgram(name, width)
    for kind, values in sends:
        it.send(kind, values, V.main(0))
    for kind, values in receives:
        it.receive(kind, values, V.main(0))
    return A.AirProgram(name, width), it


def _buses(api, chips, **kw):
    """chips: [(air, it, canonical rows)] -> (api.check_interactions, machine_check.bus_imbalance of the same tables)."""
    dev = [(a, it, _upload(api, T.monty(rows)), None) for a, it, rows in chips]
    want = MC.bus_imbalance([(it, None, np.asarray(rows, dtype=np.uint64)) for _, it, rows in chips])
    return api.check_interactions(dev, **kw), want


def test_one_bucket_hit_by_every_lane_with_different_multiplicities(api):
    h = 130
    rows = np.stack([np.arange(1, h + 1), np.full(h, 9)], axis=1)                     # every row sends (3, 7) with multiplicity row + 1
    sender = _bus_chip("S", sends=[(3, [V.const(7)])]) + (rows,)
    got, want = _buses(api, [sender])
    assert want == {(3, 7): h * (h + 1) // 2} and got["imbalance"] == want and not got["balanced"] and got["records_wanted"] == h
    same = np.stack([np.full(h, 5), np.full(h, 9)], axis=1)                           # ... and with one multiplicity in every lane
    got, want = _buses(api, [_bus_chip("S", sends=[(3, [V.const(7)])]) + (same,)])
    assert got["imbalance"] == want == {(3, 7): 5 * h}
    receiver = _bus_chip("R", receives=[(3, [V.const(7)])]) + (np.array([[h * (h + 1) // 2, 0]]),)
    got, want = _buses(api, [sender, receiver])
    assert want == {} and got["balanced"] and got["imbalance"] == {} and got["messages"] == h + 1


def test_a_multiplicity_of_p_minus_1(api):
    rows = np.array([[P - 1, 4], [0, 5], [2, 4]])
    got, want = _buses(api, [_bus_chip("S", sends=[(2, [V.main(1)])]) + (rows,)])
    assert want == {(2, 4): 1} and got["imbalance"] == want and got["messages"] == 2
    got, want = _buses(api, [_bus_chip("S", sends=[(2, [V.main(1)])]) + (rows,), _bus_chip("R", receives=[(2, [V.main(1)])]) + (np.array([[1, 4]]),)])
    assert want == {} and got["balanced"]
    got, want = _buses(api, [_bus_chip("S", sends=[(2, [V.main(1)])]) + (np.array([[P - 1, 4]]),)])
    assert want == {(2, 4): P - 1} and got["imbalance"] == want and got["records"][0].tolist() == [0, 0, 0, P - 1]


def test_messages_that_cancel_only_across_chips(api):
    values = np.arange(100, 165)
    a = _bus_chip("A", sends=[(4, [V.main(1), V.const(1)])]) + (np.stack([np.full(65, 2), values], axis=1),)
    b = _bus_chip("B", receives=[(4, [V.main(1), V.const(1)])]) + (np.stack([np.full(65, 1), values], axis=1),)
    c = _bus_chip("C", receives=[(4, [V.main(1) * 2 + (-100), V.const(1)])]) + (np.stack([np.full(65, 1), (values + 100) * pow(2, -1, P) % P], axis=1),)
    for chips, balanced in (([a], False), ([a, b], False), ([a, b, c], True), ([c, b, a], True)):
        got, want = _buses(api, chips)
        assert got["imbalance"] == want and got["balanced"] == balanced == (want == {})


@pytest.fixture(scope="module")
def haystack():
    """Two 100,000-row chips (this test's own size: a needle in that much hay): A sends (6, v, v + 1) for v = 0 .. 99,999, B receives
    the same — but for one row, whose second value is off by one."""
    n = 100_000
    v = np.arange(n)
    a = _bus_chip("A", sends=[(6, [V.main(1), V.main(1) + 1])]) + (np.stack([np.ones(n, np.int64), v], axis=1),)
    it = A.InteractionProgram("B", 3)
    it.receive(6, [V.main(1), V.main(2)], V.main(0))
    rows = np.stack([np.ones(n, np.int64), v, v + 1], axis=1)
    rows[77_777, 2] += 1
    return [a, (A.AirProgram("B", 3), it, rows)]


def test_one_unbalanced_message_among_100000(api, haystack):
    got, want = _buses(api, haystack)
    assert want == {(6, 77777, 77778): 1, (6, 77777, 77779): P - 1}
    assert got["imbalance"] == want and not got["balanced"] and not got["truncated"] and got["messages"] == 200_000
    # two unbalanced keys, two buckets per table; a balanced key shares one of them with probability 2 x 10^5 / 2^22 = 0.05 (its
    # send and its receive would be two more records each)
    assert got["nonzero_buckets"] == (2, 2) and got["records_wanted"] in (2, 4, 6)


def test_a_cap_below_the_records_wanted(api, haystack):
    got, _ = _buses(api, haystack, cap=1)
    assert got["truncated"] and not got["balanced"] and got["records_wanted"] >= 2 and len(got["records"]) == 1
    assert got["records"][0, 0] in (0, 1) and got["records"][0, 3] == 1                 # an arbitrary one of them
    got, _ = _buses(api, haystack, cap=0)
    assert got["truncated"] and not got["balanced"] and len(got["records"]) == 0 and got["imbalance"] == {}


def test_16_buckets_give_the_same_exact_dictionary(api, haystack):
    fine, want = _buses(api, haystack)
    coarse, _ = _buses(api, haystack, log_buckets=4, cap=1 << 17)
    assert coarse["imbalance"] == fine["imbalance"] == want and not coarse["balanced"] and not coarse["truncated"]
    assert 1 <= coarse["nonzero_buckets"][0] <= 2 and coarse["records_wanted"] > 2000 > fine["records_wanted"]      # false positives, filtered by the exact tally


# ---- the whole run ------------------------------------------------------------------------------------------------------------------------
def test_prove_program_check(api, tmp_path, monkeypatch, capsys):
    import ed_u256_cases as EU
    import prove_program
    elf = tmp_path / "carry.elf"
    elf.write_bytes(EU.carry_program())
    runs, proofs = {}, {}
    prove = api.ProvingKey.prove_shard

    def recording(self, *a, **k):                                         # the proofs themselves: the driver prints none of their bytes
        proof = prove(self, *a, **k)
        proofs[flags].append(hashlib.sha256(proof).hexdigest())
        return proof
    monkeypatch.setattr(api.ProvingKey, "prove_shard", recording)
    try:
        for flags in ((), ("--check",)):
            proofs[flags] = []
            monkeypatch.setattr(sys, "argv", ["prove_program.py", "--elf", str(elf), "--device-shard", "--verify"] + list(flags))
            capsys.readouterr()
            prove_program.main()
            runs[flags] = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    finally:
        api.check(api._L().sp1hip_timers_enable(0))                       # the driver's stage clocks: not the next test's business
    plain, checked = runs[()], runs[("--check",)]
    assert len(checked["per_shard"]) == len(plain["per_shard"]) >= 3
    for a, b in zip(plain["per_shard"], checked["per_shard"]):
        assert "check" not in a and "check_ms" not in a and b["check"] == "ok" and b["check_ms"] > 0
        assert a["proof_bytes"] == b["proof_bytes"]
    assert len(proofs[()]) >= len(plain["per_shard"]) and proofs[()] == proofs[("--check",)]      # every proof of the run, the same bytes
    assert all(v["rc"] == 0 for v in checked["verified_first_of_kind"].values()) and checked["whole_run"]
