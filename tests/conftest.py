"""pytest configuration: markers, paths, shared helpers."""

import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


#: largest stored fixture file: no committed file may exceed 1 MiB, a larger fixture is stored in parts
PART_BYTES = 1000 * 1000


def golden_files(path):
    """``x.npz`` itself, else the parts ``x.part0.npz``, ``x.part1.npz``, ... it is stored as ([] if neither exists)."""
    if os.path.exists(path):
        return [path]
    parts = []
    while os.path.exists(f"{path[:-4]}.part{len(parts)}.npz"):
        parts.append(f"{path[:-4]}.part{len(parts)}.npz")
    return parts


def load_npz(path):
    """Every array of fixture ``path`` (one file or its parts); an array stored as row blocks ``key#0``, ``key#1``, ...
    comes back whole."""
    out, blocks = {}, {}
    for p in golden_files(path):
        with np.load(p) as f:
            for k in f.files:
                if "#" in k:
                    key, i = k.rsplit("#", 1)
                    blocks.setdefault(key, {})[int(i)] = f[k]
                else:
                    out[k] = f[k]
    for key, b in blocks.items():
        out[key] = np.concatenate([b[i] for i in range(len(b))], axis=0)
    if not out:
        raise FileNotFoundError(path)
    return out


def save_npz_parts(path, arrays, limit=PART_BYTES, compressed=True):
    """Write ``arrays`` to ``path`` when they fit in ``limit`` bytes, else to ``x.part0.npz``, ``x.part1.npz``, ... of at
    most ``limit`` bytes each (an array larger than one part goes in row blocks ``key#0``, ``key#1``, ...)."""
    save = np.savez_compressed if compressed else np.savez
    head = 1024                                         # zip entry + .npy header of one array, generously
    items = [(k, np.asarray(v)) for k, v in arrays.items()]
    if sum(v.nbytes + head for _, v in items) <= limit:
        save(path, **dict(items))
        return [path]
    pieces = []
    for k, v in items:
        if v.ndim == 0 or v.nbytes + head <= limit:
            pieces.append((k, v))
        else:
            rows = max(1, (limit - head) // max(1, v.nbytes // v.shape[0]))
            pieces += [(f"{k}#{j}", v[r:r + rows]) for j, r in enumerate(range(0, v.shape[0], rows))]
    parts, cur, size = [], {}, 0
    for k, v in pieces:
        if cur and size + v.nbytes + head > limit:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = v
        size += v.nbytes + head
    parts.append(cur)
    out = [f"{path[:-4]}.part{i}.npz" for i in range(len(parts))]
    for p, arrs in zip(out, parts):
        save(p, **arrs)
    return out


def load_golden(name):
    return load_npz(os.path.join(GOLDEN, name + ".npz"))


def sign_align(w, ref):
    """Flip each column of ``w`` to the sign of its inner product with ``ref``."""
    s = np.sign(np.sum(w * ref, axis=0))
    s[s == 0] = 1.0
    return w * s


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def col_rel_err(w, ref):
    """Largest per-column relative error after sign alignment."""
    w = sign_align(np.asarray(w, dtype=np.float64), np.asarray(ref, dtype=np.float64))
    num = np.linalg.norm(w - ref, axis=0)
    den = np.maximum(np.linalg.norm(ref, axis=0), 1e-300)
    return float((num / den).max())


@pytest.fixture(scope="session")
def golden():
    return load_golden


def host_solve_cached(tag, probe, compute):
    """The slow part of the full-size GPU parity tests is not the GPU: it is the ORACLE's dense host solve (LAPACK on
    8192 x 8192 pencils, 40-60 s each) of float64 moments that a deterministic generator reproduces bit for bit.  Its
    result is kept as a fixture (``tests/golden/fullsize/<tag>.npz`` or its parts, weights stored as float32: 6e-8 relative, the tests
    compare at 1e-5 .. 1e-2) together with a probe of the moments it was computed from; a test first checks that ITS
    moments match the probe (else the fixture is not this data's and the oracle runs live).  ``compute()`` returns a dict
    of arrays.  Fixtures are written by ``tools/gen_golden_fullsize.sh`` (the same tests with CCZ_WRITE_FULLSIZE_GOLDEN
    set to an output directory, on a GPU box)."""
    path = os.path.join(GOLDEN, "fullsize", tag + ".npz")
    probe = np.asarray(probe, dtype=np.float64)
    if golden_files(path) and not os.environ.get("CCZ_WRITE_FULLSIZE_GOLDEN"):
        f = load_npz(path)
        if f["probe"].shape == probe.shape and np.allclose(f["probe"], probe, rtol=1e-11, atol=0.0):
            return {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in f.items() if k != "probe"}
    out = compute()
    dest = os.environ.get("CCZ_WRITE_FULLSIZE_GOLDEN")
    if dest:
        os.makedirs(dest, exist_ok=True)
        small = {k: (np.asarray(v, dtype=np.float32) if np.asarray(v).ndim == 2 else np.asarray(v)) for k, v in out.items()}
        save_npz_parts(os.path.join(dest, tag + ".npz"), dict(probe=probe, **small), compressed=False)
    return {k: np.asarray(v, dtype=np.float64) if np.asarray(v).dtype.kind == "f" else np.asarray(v) for k, v in out.items()}


def moments_probe(G, s):
    """A few numbers that pin float64 moments [G | s] (trace, corners, one interior entry, the sum of the column sums)."""
    D = G.shape[0]
    return [float(np.trace(G)), float(G[0, 0]), float(G[D - 1, D - 1]), float(G[D // 2, D // 3]), float(G[1, D - 2]), float(np.sum(s))]
