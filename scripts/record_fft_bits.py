"""Developer tool (GPU box): record tests/golden/fft_bits.json - the SHA-256 digests of the results of tests/fft_bits_cases.py - from
the library of a reference revision.  Run once per refactor of fft.hip, against its PARENT:
    scripts/build_rev.sh parent <rev>
    RMHIP_LIBRARY=ab_old/parent/librmhip.so python scripts/record_fft_bits.py <rev> [out.json]
The file's header names the revision and the date; a digest the tree then misses is a finding about the tree, not a reason to re-record."""
import datetime
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(1, str(ROOT / "tests"))
from runmat_amd import HipProvider  # noqa: E402
import fft_bits_cases  # noqa: E402

rev = sys.argv[1]
out = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "fft_bits.json"
provs = {}
got = fft_bits_cases.digests(lambda precision: provs.setdefault(precision, HipProvider(0, precision=precision)))
for p in provs.values():
    p.close()
lib = os.environ.get("RMHIP_LIBRARY")
doc = {"recorded_from": rev, "library": os.path.relpath(lib, ROOT) if lib else "in-tree", "date": datetime.date.today().isoformat(),
       "device": "MI355X (gfx950)", "digests": got}
out.parent.mkdir(parents=True, exist_ok=True)
out.write_text(json.dumps(doc, indent=1) + "\n")
print(f"{len(got)} digests from {rev} -> {out}")
