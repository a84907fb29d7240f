"""The runtime switches of libccz live in ONE table (cca_zoo_amd/csrc/env.h); this keeps it that way.

Host-only: the table and the sources are read as text, nothing is compiled."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cca_zoo_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")

ROW = re.compile(r'^\s*X\((\w+),\s*(INT|I64|REAL|FLAG|STR),\s*([^,]+),\s*(ONCE|LIVE|LOAD|HANDLE),\s*"([^"]+)"\)', re.M)

# names that Python code reads (the package, the build, the test harness), not libccz
PYTHON_SIDE = re.compile(r"CCZ_(TORCHLESS|DEVICE|FORCE_BUILD|HOSTSIM_SANITIZE|WRITE_FULLSIZE_GOLDEN|BENCH_\w+)$")

# Read once per process and yet set with monkeypatch.setenv by a test that starts no child: that test's docstring says so
# itself ("the second variant is only exercised when this test runs first in a fresh process").
SET_IN_PROCESS_THOUGH_ONCE = {"CCZ_GEMM_NN_IMPL": "test_gpu_ops.py::test_transform_f32_wide_output_kernels"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _table():
    rows = ROW.findall(_read(os.path.join(CSRC, "env.h")))
    assert len(rows) >= 59, "the table of env.h no longer parses: %d rows" % len(rows)
    return rows


def _sources():
    return sorted(p for ext in ("hip", "cpp", "h") for p in glob.glob(os.path.join(CSRC, "*." + ext)))


def test_the_table_is_well_formed():
    rows = _table()
    ids = [r[0] for r in rows]
    assert len(ids) == len(set(ids)), sorted(i for i in set(ids) if ids.count(i) > 1)
    n_rows = len(re.findall(r"^\s*X\(", _read(os.path.join(CSRC, "env.h")), flags=re.M))
    assert n_rows == len(rows), "a row of the table does not have the form X(id, kind, default, when, \"text\")"
    for ident, kind, dflt, when, doc in rows:
        # values -- consumer: class
        assert re.search(r" -- \w+\.(hip|cpp)\b.*: (knob|A/B|test|trace)\b", doc), (ident, doc)
        consumers = re.findall(r"\b(\w+\.(?:hip|cpp))\b", doc.split(" -- ", 1)[1])
        for c in consumers:
            assert re.search(r"\benv::%s\b" % ident, _read(os.path.join(CSRC, c))) or ident == "GRAM_PARTIAL_MB", (ident, c)
        assert (dflt.strip() == "nullptr") == (kind == "STR") and (dflt.strip() == "false") == (kind == "FLAG"), (ident, kind, dflt)


def test_getenv_only_in_env_h():
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if name == "env.h" or not os.path.isfile(path):
            continue
        assert not re.search(r"\bgetenv\b", _read(path)), "%s reads the environment by itself: add a row to env.h" % name


def test_every_switch_named_in_the_sources_is_declared_once():
    declared = ["CCZ_" + r[0] for r in _table()]
    for path in _sources():
        text = _read(path)
        for lit in re.findall(r'"(CCZ_[A-Z0-9_]+)"', text):
            assert declared.count(lit) == 1, "%s: \"%s\" is not a row of env.h" % (os.path.basename(path), lit)
    used = set()                                          # every row has a site (the compiler sees to the converse)
    for path in _sources():
        used.update(re.findall(r"\benv::([A-Z][A-Z0-9_]+)\b", _read(path)))
    used.update(re.findall(r"\bonce\(([A-Z][A-Z0-9_]+)\)", _read(os.path.join(CSRC, "env.h"))))
    assert sorted(used) == sorted(r[0] for r in _table()), "rows without a site, or sites without a row"


def _test_functions(text):
    """(name, body) of the top-level functions of a test module"""
    parts = re.split(r"^(?=def |@pytest|class )", text, flags=re.M)
    out = []
    for p in parts:
        m = re.match(r"def (\w+)\(", p)
        if m:
            out.append((m.group(1), p))
    return out


def test_switches_that_the_tests_set_are_declared_with_the_timing_the_tests_need():
    when = {"CCZ_" + r[0]: r[3] for r in _table()}
    setting = [r"setenv\(\s*[\"'](CCZ_\w+)[\"']", r"environ\[[\"'](CCZ_\w+)[\"']\]\s*=", r"[\"'](CCZ_\w+)[\"']\s*:",
               r"\b(CCZ_[A-Z0-9_]+)\s*=\s*[\"']"]
    seen = 0
    for path in sorted(glob.glob(os.path.join(TESTS, "*.py"))):
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue
        text = _read(path)
        for pat in setting:
            for name in re.findall(pat, text):
                if PYTHON_SIDE.match(name):
                    continue
                seen += 1
                assert name in when, "%s sets %s, which libccz does not read" % (os.path.basename(path), name)
        for fn, body in _test_functions(text):
            if "subprocess" in body:
                continue                                  # the measurement runs in a child that inherits the variable
            for name in re.findall(r"monkeypatch\.setenv\(\s*[\"'](CCZ_\w+)[\"']", body):
                if PYTHON_SIDE.match(name):
                    continue
                if name in SET_IN_PROCESS_THOUGH_ONCE:
                    assert SET_IN_PROCESS_THOUGH_ONCE[name] == "%s::%s" % (os.path.basename(path), fn)
                    assert when[name] == "ONCE"
                    continue
                assert when[name] == "LIVE", "%s::%s sets %s in its own process, but env.h reads it %s" % (
                    os.path.basename(path), fn, name, when[name])
    assert seen >= 20, "the patterns above no longer find the tests' switches (%d)" % seen
