"""Developer tool (GPU box): achieved GB/s of modulate_constellation and modulate_bits_constellation against their byte models, beside the library's own fused sin(A).*B+C at an equal byte count.
usage: modulation_rates.py [--reps N] [--log2n K] [--f32]
Both hooks are timed over 2^K input elements (default 26) for order 4, order 64 and the first order whose table is read from global
memory instead of LDS (MOD_TABLE_LDS_BYTES / 16 + 1, read from the source), plus 4096.  Byte model: symbols 8 B in + 16 B out per
sample (4 + 16 with --f32); bits 8 * bps B in + 16 B out per symbol (bps = ceil(log2(order)), symbols uniform below the order).  The
yardstick is rmhip_fused_elementwise on the planner's sin(A).*B+C request, 32 B per element (16 with --f32), sized to move the same
number of bytes as the hook beside it.  Timed with device events on the library's stream after warming every call; each figure
includes the hook's table upload and its one verdict read.  Prints one JSON line per case."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from planner_requests import sin_mul_add_plan  # noqa: E402
from runmat_amd import HipProvider  # noqa: E402


def lds_orders():
    text = open(os.path.join(ROOT, "runmat_amd", "csrc", "modulate_check.h")).read()
    return int(re.search(r"constexpr\s+\w+\s+MOD_TABLE_LDS_BYTES\s*=\s*(\d+)\s*;", text).group(1)) // 16


def main():
    args = sys.argv[1:]
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 10
    n = 1 << (int(args[args.index("--log2n") + 1]) if "--log2n" in args else 26)
    f32 = "--f32" in args
    word = 4 if f32 else 8
    p = HipProvider(0, precision="F32" if f32 else "F64")
    plan, out_id = sin_mul_add_plan()
    shader = plan.generate_wgsl_for_output(out_id, "f32" if f32 else "f64")
    rng = np.random.default_rng(11)

    def timed(fn):
        for _ in range(2):
            fn()
        p.timer_begin()
        for _ in range(reps):
            fn()
        return p.timer_end() / reps

    def yardstick(nbytes):
        m = max(int(nbytes // (4 * word)), 1)
        ops = [p.upload(rng.uniform(-1.0, 1.0, m), (m, 1)) for _ in range(3)]
        ms = timed(lambda: p.free(p.fused_elementwise(shader, ops, (m, 1), m)))
        for h in ops:
            p.free(h)
        return ms, 4 * word * m

    first_global = lds_orders() + 1
    for order in (4, 64, first_global, 4096):
        table = rng.standard_normal(2 * order)
        bps = max(int(np.ceil(np.log2(order))), 1)
        # symbols
        h = p.upload(rng.integers(0, order, n).astype(np.float64), (n, 1))
        ms = timed(lambda: p.free(p.modulate_constellation(h, table)))
        p.free(h)
        nbytes = n * (word + 16)
        yms, ybytes = yardstick(nbytes)
        print(json.dumps({"hook": "modulate_constellation", "storage": "f32" if f32 else "f64", "order": order, "samples": n, "table": "lds" if order < first_global else "global",
                          "ms": round(ms, 4), "model_bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1), "fused_ms": round(yms, 4),
                          "fused_GBps": round(ybytes / yms / 1e6, 1), "ratio_to_fused": round((nbytes / ms) / (ybytes / yms), 3)}), flush=True)
        # bits: n input elements, n // bps symbols
        groups = n // bps
        symbols = rng.integers(0, order, groups).astype(np.uint64)
        bits = ((symbols[:, None] >> np.arange(bps - 1, -1, -1, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64).reshape(-1)
        h = p.upload(bits, (groups * bps, 1))
        ms = timed(lambda: p.free(p.modulate_bits_constellation(h, groups * bps, bps, table)))
        p.free(h)
        nbytes = groups * (word * bps + 16)
        yms, ybytes = yardstick(nbytes)
        print(json.dumps({"hook": "modulate_bits_constellation", "storage": "f32" if f32 else "f64", "order": order, "bps": bps, "symbols": groups,
                          "table": "lds" if order < first_global else "global", "ms": round(ms, 4), "model_bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1),
                          "fused_ms": round(yms, 4), "fused_GBps": round(ybytes / yms / 1e6, 1), "ratio_to_fused": round((nbytes / ms) / (ybytes / yms), 3)}), flush=True)
    p.close()


if __name__ == "__main__":
    main()
