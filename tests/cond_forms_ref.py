"""Cases and CPU references shared by tests/test_cond_forms_host.py and tests/test_gpu_cond_forms.py: `cond(A, p)` for p = one, inf, fro
(rmhip_cond_norm) and linsolve's rcond (rmhip_linsolve_rcond).

The cond reference is composed from what oracle/ restates - norm(A, p) * norm(inv(A), p) with cond.rs's rules around it (cond.rs:276-300,
343-357, 384-414); a second CPU evaluation (numpy's LAPACK inverse and norms) measures how far two correct evaluations lie apart.  The
rcond reference is sigma_min / sigma_max of numpy's SVD with the zero and non-finite rules of singular_value_rcond
(common/linalg.rs:241-259)."""
import re
from collections import namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
EPS = float(np.finfo(float).eps)
NORMS = ("one", "inf", "fro")
KINDS = ("dominant", "plain", "scaled")
SQUARE_TEXT = "cond: matrix must be square for the requested norm."
SINGULAR_TEXT = "linsolve: matrix is singular to working precision."
GOLDEN = ROOT / "tests" / "golden" / "cond_forms_ref.json"
LIVE_MAX = 130  # orders up to here are recomputed by the oracle wherever a reference is needed

Case = namedtuple("Case", "name a")


def slab_cols() -> int:
    """kCondSlabCols as the source states it: the orders around it are where the slab loop takes another path."""
    m = re.search(r"constexpr int kCondSlabCols = (\d+);", (ROOT / "runmat_amd" / "csrc" / "cond_norm.hip").read_text())
    assert m, "kCondSlabCols is not a single constexpr in cond_norm.hip"
    w = int(m.group(1))
    assert 1 <= w <= 1024
    return w


def orders():
    w = slab_cols()
    return sorted({2, 3, 5, 17, 64, 65, 130, w - 1, w, w + 1, 2 * w + 3})


def matrix(n: int, kind: str) -> np.ndarray:
    u = np.random.default_rng(1000 * n + KINDS.index(kind)).uniform(-1.0, 1.0, (n, n))
    if kind == "dominant":
        return u + n * np.eye(n)
    if kind == "scaled":
        return u * np.logspace(0.0, -6.0, n)[None, :]
    return u


def case_keys():
    return [(n, kind) for n in orders() for kind in KINDS]


def case(n: int, kind: str) -> Case:
    return Case(f"{kind}{n}", matrix(n, kind))


def generated():
    """One case at a time: the largest matrices are 32 MiB each."""
    for n, kind in case_keys():
        yield case(n, kind)


# cond.rs:661-690 (the reference's own KATs), then the singular matrices: (name, matrix, norm, value)
EXACT = [
    ("kat_one", np.array([[4.0, -1.0], [2.0, 3.0]]), "one", 15.0 / 7.0),
    ("kat_inf", np.array([[4.0, -1.0], [2.0, 3.0]]), "inf", 15.0 / 7.0),
    ("kat_fro", np.diag([5.0, 2.0]), "fro", 2.9),
]
SINGULAR = [("ones3", np.ones((3, 3))), ("rank1", np.array([[1.0, 2.0], [2.0, 4.0]])), ("zeros4", np.zeros((4, 4)))]
TINY_PIVOT = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]])  # the last pivot is rounding noise, not zero: declined
NON_SQUARE = np.arange(6.0).reshape(2, 3)
SCALARS = [(0.0, np.inf), (2.0, 1.0), (np.nan, 1.0)]


def with_inf() -> np.ndarray:
    a = matrix(5, "dominant").copy()
    a[3, 1] = np.inf
    return a


def _finish(v: float) -> float:
    return float(v) if np.isfinite(v) else float("inf")


def cond_ref(oracle, a: np.ndarray, norm: str) -> float:
    """cond.rs:276-300, 343-357, 384-414 over oracle.norm and oracle.inv."""
    a = np.asarray(a, dtype=np.float64)
    rows, cols = (a.shape[0] if a.ndim >= 1 else 1), (a.shape[1] if a.ndim >= 2 else 1)
    if rows == 0 or cols == 0:
        return 0.0
    if rows == 1 and cols == 1:
        return float("inf") if a.reshape(-1)[0] == 0.0 else 1.0
    if rows != cols:
        raise ValueError(SQUARE_TEXT)
    return cond_ref_all(oracle, a)[norm]


def cond_ref_all(oracle, a: np.ndarray) -> dict:
    """The three norms of a square matrix of order >= 2 from one inverse."""
    inv = oracle.inv(a)
    if inv is None:
        return {norm: float("inf") for norm in NORMS}
    return {norm: _finish(oracle.norm(a, norm) * oracle.norm(inv, norm)) for norm in NORMS}


def cond_numpy(a: np.ndarray, norm: str) -> float:
    """The second CPU evaluation: LAPACK's inverse, numpy's norms."""
    order = {"one": 1, "inf": np.inf, "fro": "fro"}[norm]
    return _finish(np.linalg.norm(a, order) * np.linalg.norm(np.linalg.inv(a), order))


def checksum(a: np.ndarray) -> str:
    """Ties a recorded value to the matrix it was computed from."""
    return float(np.sum(a * np.arange(1.0, a.size + 1.0).reshape(a.shape))).hex()


def recorded() -> dict:
    """case name -> {norm: cond_ref's value}: the oracle's values as `python tests/cond_forms_ref.py --record` wrote them to
    tests/golden/cond_forms_ref.json.  The oracle's inverse is a single-threaded n^3 loop - 36 s per matrix at n = 2051 - so the tests read
    the large orders from this file; tests/test_cond_forms_host.py recomputes every order up to LIVE_MAX and checks the file bit for
    bit against it, and checks every entry against the matrix and slab width of today."""
    import json

    doc = json.loads(GOLDEN.read_text())
    assert doc["slab_cols"] == slab_cols(), "kCondSlabCols changed: record tests/golden/cond_forms_ref.json again"
    out = {}
    for case in generated():
        entry = doc["cases"].get(case.name)
        assert entry and entry["checksum"] == checksum(case.a), f"{case.name}: record tests/golden/cond_forms_ref.json again"
        out[case.name] = {norm: float.fromhex(entry[norm]) for norm in NORMS}
    return out


def record():
    import json
    import sys

    sys.path.insert(0, str(ROOT))
    from oracle import oracle

    cases = {}
    for case in generated():
        cases[case.name] = {"n": case.a.shape[0], "checksum": checksum(case.a), **{norm: v.hex() for norm, v in cond_ref_all(oracle, case.a).items()}}
        print(case.name, cases[case.name], flush=True)
    GOLDEN.write_text(json.dumps({"slab_cols": slab_cols(), "cases": cases}, indent=1) + "\n")


def gate(n: int, ref: float) -> float:
    """n eps kappa_p ref with kappa_p = ref: the first-order forward bound of an LU inverse, constant 1."""
    return n * EPS * ref * ref


def rcond_ref(a: np.ndarray) -> float:
    s = np.linalg.svd(np.asarray(a, dtype=np.float64), compute_uv=False)
    if not np.isfinite(s).all() or s.max() == 0.0:
        return 0.0
    return float(s.min() / s.max())


def rank_deficient(n: int = 20, r: int = 10) -> np.ndarray:
    rng = np.random.default_rng(n * r)
    return rng.standard_normal((n, r)) @ rng.standard_normal((r, n))


if __name__ == "__main__":
    import sys

    if "--record" in sys.argv[1:]:
        record()
