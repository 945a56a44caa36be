"""CPU: the row rounds of a LogUp-GKR layer in closed form (sp1_amd/csrc/gkr_rounds_host.hpp, which the prover runs between two
hand-overs), by the host program tests/native/gkr_rounds: no GPU, no library.

For k = 1 .. 4 rounds per pass and 0 .. 2 further unbound row variables, on random layers whose interactions end inside a cell,
are shorter than one cell (whole cells of padding) or have no rows: the 3^k + 1 grid sums are computed from the definition (every
table of a cell on {0, 1, inf}^k, axis by axis), the closed form turns them into k cubics, and every cubic equals the round
polynomial of the sumcheck — the sum over the remaining hypercube of eq F with the earlier variables at their challenges — at
0, 1, 2 and 3; the running claim chains from round to round; the eq factor of the bound variables comes back; and for k <= 2 the
general form gives the words of the two-round pass's own function. Field elements: exact equality."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "native", "gkr_rounds")

# 12 cases (k, extra); per case: the round count, 6 checks per round, the eq factor, and for k <= 2 the two-round comparison
CHECKS = sum(1 + 6 * k + 1 + (1 if k <= 2 else 0) for k in (1, 2, 3, 4) for _ in range(3))


@pytest.fixture(scope="module", autouse=True)
def _program():
    assert os.path.exists(EXE), "tests/native/gkr_rounds is not built: run __graft_entry__.build()"


@pytest.mark.parametrize("seed", [1, 2, 20261020])
def test_closed_form_rounds_equal_the_definition(seed):
    r = subprocess.run([EXE, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert not [ln for ln in lines if ln.startswith("FAIL")], r.stdout
    assert [ln for ln in lines if ln.startswith("case")] == ["case k = %d, t = %d: done" % (k, k + e) for k in (1, 2, 3, 4) for e in (0, 1, 2)]
    assert lines[-1] == "OK %d" % CHECKS
