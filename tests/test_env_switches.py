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

# how a test sets a switch: monkeypatch.setenv / os.environ[...] = / an environment dict of a child / a shell-style assignment
SETTING = [r"setenv\(\s*[\"'](CCZ_\w+)[\"']", r"environ\[[\"'](CCZ_\w+)[\"']\]\s*=", r"[\"'](CCZ_\w+)[\"']\s*:",
           r"\b(CCZ_[A-Z0-9_]+)\s*=\s*[\"']"]

# Rows (or the part of a row) that no test sets, each with its reason.  A new row lands either with a test that sets it or here.
NOT_EXERCISED = {
    "CCZ_RCCL_LIB": "tests force the not-found path with it; the found path needs an RCCL library and more than one GPU",
}


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
    seen = 0
    for path in sorted(glob.glob(os.path.join(TESTS, "*.py"))):
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue
        text = _read(path)
        for pat in SETTING:
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
                assert when[name] == "LIVE", "%s::%s sets %s in its own process, but env.h reads it %s" % (
                    os.path.basename(path), fn, name, when[name])
    assert seen >= 20, "the patterns above no longer find the tests' switches (%d)" % seen


def test_every_switch_is_set_by_some_test():
    """The ratchet: every row of the table is set by a test (found with the patterns above) or named in NOT_EXERCISED with its
    reason -- a switch is a second code path, and a path no test takes can be wrong, read out of bounds or never finish
    without any run showing it."""
    declared = ["CCZ_" + r[0] for r in _table()]
    set_by = {}
    for path in sorted(glob.glob(os.path.join(TESTS, "*.py"))):
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue
        text = _read(path)
        for pat in SETTING:
            for name in re.findall(pat, text):
                set_by.setdefault(name, os.path.basename(path))
    assert sorted(n for n in NOT_EXERCISED if n not in declared) == [], "NOT_EXERCISED names rows that env.h does not have"
    assert all(len(reason.strip()) > 10 for reason in NOT_EXERCISED.values())
    missing = sorted(n for n in declared if n not in set_by and n not in NOT_EXERCISED)
    assert missing == [], "switches that no test sets: give each a test, or a line in NOT_EXERCISED: %s" % missing
