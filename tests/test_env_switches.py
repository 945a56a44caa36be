"""The SP1HIP_* environment switches: the set the native library reads equals the set INTEGRATION.md documents, and the
switches that were removed (prover forms that lost their A/B run, tuning knobs nobody set) stay removed everywhere."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# getenv, or one of the helpers of sp1_amd/csrc/common.hpp, on a literal name
READ = re.compile(r'\b(?:getenv|env_flag|env_uint)\(\s*"(SP1HIP_[A-Z0-9_]+)"')

REMOVED = {
    "SP1HIP_ZC_FUSE_NODES", "SP1HIP_ZC_BIV_CORNERS", "SP1HIP_ZC_GROUPS", "SP1HIP_ZC_WG", "SP1HIP_ZC_POLY_WAVE", "SP1HIP_ZC_MONO",
    "SP1HIP_ZC_FINE", "SP1HIP_ZC_MAD", "SP1HIP_ZC_MADC", "SP1HIP_ZC_SCHEDULE", "SP1HIP_JAGGED_COL_SLICE", "SP1HIP_NTT_GENERIC",
    "SP1HIP_NTT_PLAN", "SP1HIP_ZC_LAZY_MIN_REGS", "SP1HIP_ZC_CHUNK_LIMIT", "SP1HIP_ZC_CHUNK_HARD_MAX", "SP1HIP_ZC_MAX_PAIRS",
    "SP1HIP_ZC_FORK_MAX_BLOCKS", "SP1HIP_ZC_NFORK", "SP1HIP_GKR_TILES", "SP1HIP_GATE", "SP1HIP_GATE_MAX_TILES", "SP1HIP_ZC_KECCAK3",
}


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(*dirs):
    for d in dirs:
        for base, subdirs, names in os.walk(os.path.join(ROOT, d)):
            subdirs[:] = [s for s in subdirs if s not in ("__pycache__", "target", "lib", "golden")]
            for n in names:
                yield os.path.join(base, n)


def _switches_read_by_the_library():
    names = set()
    for path in _files(os.path.join("sp1_amd", "csrc")):
        names.update(READ.findall(_read(path)))
    return names


def _documented_list():
    """The `Environment switches` bullet of INTEGRATION.md: from its first line to the next top-level bullet or heading."""
    lines = _read(os.path.join(ROOT, "INTEGRATION.md")).split("\n")
    start = [i for i, ln in enumerate(lines) if ln.startswith("* **Environment switches.**")]
    assert len(start) == 1, "INTEGRATION.md has exactly one `Environment switches` list"
    end = next(i for i in range(start[0] + 1, len(lines)) if lines[i].startswith(("* ", "#")))
    return "\n".join(lines[start[0]:end])


def test_the_documented_switches_are_the_ones_the_library_reads():
    read = _switches_read_by_the_library()
    documented = set(re.findall(r"`(SP1HIP_[A-Z0-9_]+)", _documented_list()))
    assert read, "no switch found under sp1_amd/csrc: the pattern no longer matches how they are read"
    assert read == documented, "read but not documented: %s; documented but not read: %s" % (sorted(read - documented), sorted(documented - read))
    assert not (read & REMOVED)


def test_removed_switches_are_named_nowhere():
    me = os.path.abspath(__file__)
    found = []
    texts = [(p, _read(p)) for p in _files("sp1_amd", "include", "tests", "bench", "rust") if os.path.abspath(p) != me
             and not p.endswith((".so", ".pyc", ".o"))]
    texts.append(("INTEGRATION.md (switch list)", _documented_list()))
    for path, text in texts:
        for name in set(re.findall(r"SP1HIP_[A-Z0-9_]+", text)) & REMOVED:
            found.append((os.path.relpath(path, ROOT) if os.path.isabs(path) else path, name))
    assert not found, found
