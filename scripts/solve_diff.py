"""Developer tool (GPU box): run a fixed, seeded list of systems through mldivide / mrdivide / inv / linsolve and dump, per case, the result bytes, the status and last-error text of a refusal and the telemetry deltas; compare two dumps (e.g. two builds via RMHIP_LIBRARY) for exact equality.
usage: solve_diff.py dump <out.npz>  |  solve_diff.py compare <a.npz> <b.npz>"""
import contextlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def rank_deficient(rng, m, n):
    a = rng.uniform(-1, 1, (m, n))
    a[:, -1] = a[:, 0] + a[:, 1]
    return a


def graded(rng, n, lo, hi):  # singular values from hi down to lo: nearly singular, every pivot well above 1e-12
    q1, _ = np.linalg.qr(rng.standard_normal((n, n)))
    q2, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (q1 * np.geomspace(hi, lo, n)) @ q2


def cases():
    """(name, op, operands, options, environment) - operands are built lazily, one case at a time"""
    from runmat_amd.provider import ProviderLinsolveOptions as Opt

    def sq(n, nrhs, seed):
        def make():
            rng = np.random.default_rng(seed)
            return rng.uniform(-1, 1, (n, n)) + 0.5 * np.eye(n), rng.uniform(-1, 1, (n, nrhs))
        return make

    def rect(m, n, nrhs, seed, deficient=False):
        def make():
            rng = np.random.default_rng(seed)
            return (rank_deficient(rng, m, n) if deficient else rng.uniform(-1, 1, (m, n))), rng.uniform(-1, 1, (m, nrhs))
        return make

    def sing(n, nrhs, seed):
        def make():
            rng = np.random.default_rng(seed)
            return rank_deficient(rng, n, n), rng.uniform(-1, 1, (n, nrhs))
        return make

    def tri(n, nrhs, seed, lower):
        def make():
            rng = np.random.default_rng(seed)
            a = rng.uniform(-1, 1, (n, n)) + 4.0 * np.eye(n)
            return (np.tril(a) if lower else np.triu(a)), rng.uniform(-1, 1, (n, nrhs))
        return make

    def right(make):  # the operands of B / A from those of A \\ B': (B', A)
        def flipped():
            a, b = make()
            return b.T, a
        return flipped

    out = [(f"mldivide n={n} nrhs=1", "mldivide", sq(n, 1, n), None, {}) for n in (8, 64)]
    out += [(f"mldivide n={n} nrhs={k}", "mldivide", sq(n, k, n + k), None, {}) for n in (65, 1000, 2048, 2500, 4096) for k in (1, 17)]
    out += [("mldivide rank-deficient n=32", "mldivide", sing(32, 2, 1), None, {}),
            ("mldivide rank-deficient n=300", "mldivide", sing(300, 2, 2), None, {}),
            ("mldivide rank-deficient n=32, no SVD path", "mldivide", sing(32, 2, 1), None, {"RMHIP_NO_SVD_PATH": "1"}),
            ("mldivide rank-deficient n=300, no SVD path", "mldivide", sing(300, 2, 2), None, {"RMHIP_NO_SVD_PATH": "1"}),
            ("mldivide nearly singular n=200 (ratio proxy)", "mldivide",
             lambda: (graded(np.random.default_rng(3), 200, 1e-9, 1e6), np.random.default_rng(4).uniform(-1, 1, (200, 3))), None, {}),
            ("mldivide nearly singular n=40 (ratio proxy, small solver)", "mldivide",
             lambda: (graded(np.random.default_rng(5), 40, 1e-9, 1e6), np.random.default_rng(6).uniform(-1, 1, (40, 3))), None, {}),
            ("mldivide n=48 blocked (no small solver)", "mldivide", sq(48, 2, 7), None, {"RMHIP_NO_SMALL_SOLVE": "1"}),
            ("mldivide tall skinny 2^20 x 8", "mldivide", rect(1 << 20, 8, 1, 8), None, {}),
            ("mldivide tall skinny 2^16 x 8, MFMA Gram", "mldivide", rect(1 << 16, 8, 1, 9), None, {"RMHIP_NO_GRAM_SKINNY": "1"}),
            ("mldivide tall 4096 x 512", "mldivide", rect(4096, 512, 3, 10), None, {}),
            ("mldivide wide 512 x 4096", "mldivide", rect(512, 4096, 3, 11), None, {}),
            ("mldivide rank-deficient 300 x 40", "mldivide", rect(300, 40, 2, 12, True), None, {}),
            ("mldivide rank-deficient 300 x 40, no SVD path", "mldivide", rect(300, 40, 2, 12, True), None, {"RMHIP_NO_SVD_PATH": "1"}),
            ("mldivide scalar divisor", "mldivide", lambda: (np.array([[3.0]]), np.random.default_rng(13).uniform(-1, 1, (7, 5))), None, {}),
            ("mrdivide square n=100", "mrdivide", right(sq(100, 5, 14)), None, {}),
            ("mrdivide square n=2500", "mrdivide", right(sq(2500, 2, 15)), None, {}),
            ("mrdivide scalar divisor", "mrdivide", lambda: (np.random.default_rng(16).uniform(-1, 1, (6, 9)), np.array([[-0.75]])), None, {}),
            ("mrdivide singular n=64, no SVD path", "mrdivide", right(sing(64, 2, 17)), None, {"RMHIP_NO_SVD_PATH": "1"}),
            ("inv regular n=50", "inv", sq(50, 1, 18), None, {}),
            ("inv regular n=700", "inv", sq(700, 1, 19), None, {}),
            ("inv singular n=50", "inv", sing(50, 1, 20), None, {}),
            ("inv singular n=300", "inv", sing(300, 1, 21), None, {}),
            ("inv nearly singular n=200", "inv", lambda: (graded(np.random.default_rng(22), 200, 1e-9, 1e6), None), None, {}),
            ("linsolve general n=40 (small solver)", "linsolve", sq(40, 3, 23), Opt(), {}),
            ("linsolve general n=500", "linsolve", sq(500, 3, 24), Opt(), {}),
            ("linsolve general n=2500", "linsolve", sq(2500, 2, 25), Opt(), {}),
            ("linsolve general n=500 transposed", "linsolve", sq(500, 3, 26), Opt(transposed=True), {}),
            ("linsolve general n=40 transposed (small solver)", "linsolve", sq(40, 3, 27), Opt(transposed=True), {}),
            ("linsolve nearly singular n=200 (no proxy)", "linsolve",
             lambda: (graded(np.random.default_rng(3), 200, 1e-9, 1e6), np.random.default_rng(4).uniform(-1, 1, (200, 3))), Opt(), {}),
            ("linsolve lower n=300", "linsolve", tri(300, 4, 28, True), Opt(lower=True), {}),
            ("linsolve upper n=300", "linsolve", tri(300, 4, 29, False), Opt(upper=True), {}),
            ("linsolve lower n=300 rcond", "linsolve", tri(300, 4, 28, True), Opt(lower=True, need_rcond=True, rcond=1e-6), {}),
            ("linsolve upper n=300 rcond refused", "linsolve", tri(300, 4, 29, False), Opt(upper=True, need_rcond=True, rcond=0.99), {}),
            ("linsolve lower n=300 transposed", "linsolve", tri(300, 4, 30, True), Opt(lower=True, transposed=True), {}),
            ("linsolve general rcond refused", "linsolve", sq(100, 1, 31), Opt(need_rcond=True), {}),
            ("linsolve rectangular 1000 x 50", "linsolve", rect(1000, 50, 2, 32), Opt(), {}),
            ("linsolve rectangular 50 x 1000 transposed", "linsolve", lambda: (rect(50, 1000, 2, 33)()[0], rect(1000, 50, 2, 33)()[1]), Opt(transposed=True), {}),
            ("linsolve rank-deficient 300 x 40", "linsolve", rect(300, 40, 2, 34, True), Opt(), {}),
            ("linsolve singular n=32 (small solver)", "linsolve", sing(32, 2, 35), Opt(), {}),
            ("linsolve singular n=300", "linsolve", sing(300, 2, 36), Opt(), {}),
            ("linsolve singular n=300 transposed", "linsolve", sing(300, 2, 36), Opt(transposed=True), {}),
            ("linsolve singular n=32, no SVD path", "linsolve", sing(32, 2, 35), Opt(), {"RMHIP_NO_SVD_PATH": "1"}),
            ("linsolve singular n=300, no SVD path", "linsolve", sing(300, 2, 36), Opt(), {"RMHIP_NO_SVD_PATH": "1"})]
    return out


def dump(path):
    from runmat_amd import HipProvider
    from runmat_amd.provider import ProviderError

    prov = HipProvider(0)
    arrays, meta = {}, []
    for idx, (name, op, make, opts, environ) in enumerate(cases()):
        a, b = make()
        ha = prov.upload(np.asfortranarray(a))
        hb = prov.upload(np.asfortranarray(b)) if b is not None else None
        prov.reset_telemetry()
        before = prov.lu_stats()
        rec = {"name": name, "code": 0, "message": "", "rcond": None}
        with env(**environ):
            try:
                if op == "mldivide": x = prov.mldivide(ha, hb)
                elif op == "mrdivide": x = prov.mrdivide(ha, hb)
                elif op == "inv": x = prov.inv(ha)
                else:
                    r = prov.linsolve(ha, hb, opts)
                    x, rec["rcond"] = r.solution, repr(r.reciprocal_condition)
                arrays[f"x{idx}"] = np.ascontiguousarray(prov.download(x)).view(np.uint64)
                prov.free(x)
            except ProviderError as e:
                rec["code"], rec["message"] = int(e.code), str(e)
        after, snap = prov.lu_stats(), prov.telemetry_snapshot()
        rec["solve_path_factorizations"] = int(after["solve_path_factorizations"] - before["solve_path_factorizations"])
        rec["svd_solves"] = int(after["svd_solves"] - before["svd_solves"])
        rec["solve_fallbacks"] = [list(f) for f in snap["solve_fallbacks"]]
        rec["kernel_launches"] = [k["kernel"] for k in snap["kernel_launches_log"]]
        meta.append(rec)
        prov.free(ha)
        if hb is not None:
            prov.free(hb)
        print(f"{name:58s} code {rec['code']} fast {rec['solve_path_factorizations']} svd {rec['svd_solves']} "
              f"fallbacks {rec['solve_fallbacks']} launches {len(rec['kernel_launches'])}", flush=True)
    np.savez(path, meta=np.array(json.dumps(meta)), **arrays)


def compare(pa, pb):
    da, db = np.load(pa), np.load(pb)
    ma, mb = json.loads(str(da["meta"])), json.loads(str(db["meta"]))
    bad = int(len(ma) != len(mb))
    for idx, (ra, rb) in enumerate(zip(ma, mb)):
        diffs = [k for k in ra if ra[k] != rb.get(k)]
        key = f"x{idx}"
        if (key in da.files) != (key in db.files): diffs.append("result present")
        elif key in da.files and not np.array_equal(da[key], db[key]): diffs.append("result bits")
        bad += bool(diffs)
        what = f"{da[key].size} values" if key in da.files else f"refused, code {ra['code']}"
        print(f"{'DIFF ' + str(diffs) if diffs else 'same':6s} {ra['name']:58s} {what}, {len(ra['kernel_launches'])} launches")
    print(f"{len(ma)} cases, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else compare(sys.argv[2], sys.argv[3]))
