"""Developer tool (GPU box): device pagefun(@mtimes) per tier against the per-page matmul loop, the host builtin's numpy restatement and torch.matmul - ms per call, launches, share of the tier's roofline.  Usage: pagefun_rates.py [--quick] [--torch] | --complex
(--torch adds the vendor ceiling; leave it out under a kernel tracer; --complex times rmhip_complex_pagefun per operand kind beside the real
sibling at the same shapes and nothing else)

Roofline: bytes = 8 (pages_A m k + pages_B k n + P m n), flops = 2 m n k P; the least time is the larger of bytes / 8.0 TB/s (HBM) and
flops / 78.6 TFLOP/s (fp64 MFMA dense peak, MI355X_MICROARCH); the tiny tier's VALU bound (about 39e12 f64 lane ops/s, 2 per
multiply-add) is reported beside it.  The per-page matmul loop (one launch per page, the reference's wgpu provider) is timed on at most
1e4 pages and scaled up."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np

from pagefun_host import build_request, pagefun_host
from runmat_amd import HipProvider, PagefunOp, PagefunRequest

HBM = 8.0e12
MFMA = 78.6e12
VALU = 39e12
LOOP_PAGES = 10000

# (m, k, n, pages, lhs page count) - lhs 1: the shared-lhs tier
SHAPES = [(4, 4, 4, 1000000, None), (3, 3, 3, 1000000, None), (16, 16, 16, 100000, None), (32, 32, 32, 20000, None),
          (64, 64, 64, 4096, None), (128, 128, 128, 512, None), (512, 512, 512, 64, None), (1024, 1024, 1024, 16, None),
          (8, 8, 8, 100000, 1), (256, 256, 256, 64, 1)]
if "--quick" in sys.argv:
    SHAPES = [SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[6]]


def tier_of(prov):
    log = [e for e in prov.telemetry_snapshot()["kernel_launches_log"] if e["kernel"] == "pagefun"]
    return log[-1]["tuning"]["tier"]


def device_ms(prov, fn, reps):
    fn()
    prov.synchronize()
    prov.timer_begin()
    for _ in range(reps):
        fn()
    return prov.timer_end() / reps


def complex_rates(prov):
    """--complex: rmhip_complex_pagefun per operand kind beside the real sibling at the same shape.  A complex x complex product moves
    2x the bytes (16 per element) and does 4x the real multiply-adds (8 m n k P flops); a mixed product moves (A or B doubled, C doubled)
    and does 2x.  `x_real` is the ratio of the times."""
    def operand(shape, cplx):
        hr = prov.random_uniform(shape)
        if not cplx:
            return hr
        hi = prov.random_uniform(shape)
        z = prov.complex_from_real_imag(hr, hi)
        prov.free(hr)
        prov.free(hi)
        return z

    for m, k, n, P in [(4, 4, 4, 100000), (8, 8, 8, 100000), (16, 16, 16, 100000), (32, 32, 32, 20000), (40, 40, 40, 2000), (128, 128, 128, 200),
                       (512, 512, 512, 16)]:
        r = build_request([m, k, P], [k, n, P])
        reps = 10
        ha, hb = operand([m, k, P], False), operand([k, n, P], False)
        req = PagefunRequest(PagefunOp.Mtimes, [ha, hb], r.output_shape, r.page_dims, r.input_page_dims)
        real_ms = device_ms(prov, lambda: prov.free(prov.pagefun(req)), reps)
        rec = {"shape": [m, k, n], "pages": P, "real_tier": tier_of(prov), "real_ms": round(real_ms, 4)}
        prov.free(ha)
        prov.free(hb)
        for kind, name in ((0, "cc"), (1, "cr"), (2, "rc")):
            ea, eb = (1 if kind == 2 else 2), (1 if kind == 1 else 2)
            ha, hb = operand([m, k, P], ea == 2), operand([k, n, P], eb == 2)
            req = PagefunRequest(PagefunOp.Mtimes, [ha, hb], r.output_shape, r.page_dims, r.input_page_dims)
            ms = device_ms(prov, lambda: prov.free(prov.complex_pagefun(req)), reps)
            log = [e for e in prov.telemetry_snapshot()["kernel_launches_log"] if e["kernel"] == "complex_pagefun"][-1]
            nbytes = 8.0 * P * (ea * m * k + eb * k * n + 2 * m * n)
            flops = (8.0 if kind == 0 else 4.0) * m * n * k * P
            rec[name] = {"tier": log["tuning"]["tier"], "pages_per_block": log["tuning"]["pages_per_block"], "ms": round(ms, 4),
                         "x_real": round(ms / real_ms, 2), "hbm_TBs": round(nbytes / ms / 1e9, 3), "TFLOPs": round(flops / ms / 1e9, 2),
                         "roofline_frac": round(max(nbytes / HBM, flops / MFMA) * 1e3 / ms, 3)}
            prov.free(ha)
            prov.free(hb)
        print(json.dumps(rec), flush=True)


prov = HipProvider(0)
if "--complex" in sys.argv:
    complex_rates(prov)
    prov.close()
    sys.exit(0)
for m, k, n, P, lhs_pages in SHAPES:
    pa = P if lhs_pages is None else lhs_pages
    ha = prov.random_uniform([m, k, pa])
    hb = prov.random_uniform([k, n, P])
    r = build_request([m, k, pa], [k, n, P])
    req = PagefunRequest(PagefunOp.Mtimes, [ha, hb], r.output_shape, r.page_dims, r.input_page_dims)
    reps = 10 if m * n * k * P < 2e10 else 3
    t0 = prov.telemetry_snapshot()["kernel_launches"]
    ms = device_ms(prov, lambda: prov.free(prov.pagefun(req)), reps)
    launches = (prov.telemetry_snapshot()["kernel_launches"] - t0) // (reps + 1)
    tier = tier_of(prov)
    nbytes = 8.0 * (pa * m * k + P * k * n + P * m * n)
    flops = 2.0 * m * n * k * P
    t_hbm, t_mma = nbytes / HBM, flops / MFMA
    bound = "hbm" if t_hbm >= t_mma else "mfma"
    rec = {"shape": [m, k, n], "pages": P, "lhs_pages": pa, "tier": tier, "ms": round(ms, 4), "launches": launches,
           "MB": round(nbytes / 1e6, 1), "GFLOP": round(flops / 1e9, 3), "bound": bound,
           "roofline_frac": round(max(t_hbm, t_mma) * 1e3 / ms, 3),
           "hbm_TBs": round(nbytes / ms / 1e9, 3), "TFLOPs": round(flops / ms / 1e9, 2)}
    if tier == 2:
        rec["valu_frac"] = round(flops / VALU * 1e3 / ms, 3)
    # the per-page matmul loop (one dgemm launch per page), on a bounded sample
    lp = min(P, LOOP_PAGES)
    pages_a = [prov.random_uniform([m, k]) for _ in range(min(pa, lp))]
    pages_b = [prov.random_uniform([k, n]) for _ in range(min(lp, 64))]

    def loop():
        for i in range(lp):
            prov.free(prov.matmul(pages_a[i % len(pages_a)], pages_b[i % len(pages_b)]))

    rec["loop_ms_scaled"] = round(device_ms(prov, loop, 1) * P / lp, 3)
    for h in pages_a + pages_b:
        prov.free(h)
    # the host builtin's restatement, on a sample of pages
    hp = min(P, 2000)
    A = np.random.default_rng(1).standard_normal((m, k, min(pa, hp)))
    B = np.random.default_rng(2).standard_normal((k, n, hp))
    t = time.perf_counter()
    pagefun_host(A, B)
    rec["host_numpy_ms_scaled"] = round((time.perf_counter() - t) * 1e3 * P / hp, 3)
    if "--torch" in sys.argv:
        try:
            import torch

            ta = torch.rand((pa, k, m), dtype=torch.float64, device="cuda").transpose(1, 2)
            tb = torch.rand((P, n, k), dtype=torch.float64, device="cuda").transpose(1, 2)
            torch.matmul(ta, tb)
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                torch.matmul(ta, tb)
            torch.cuda.synchronize()
            rec["torch_ms"] = round((time.perf_counter() - t) * 1e3 / reps, 4)
            del ta, tb
        except Exception as e:  # no torch / no device: the ceiling is optional
            rec["torch_error"] = str(e)[:80]
    prov.free(ha)
    prov.free(hb)
    print(json.dumps(rec), flush=True)
prov.close()
