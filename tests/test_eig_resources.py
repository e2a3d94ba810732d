"""The eig kernels (runmat_amd/csrc/eig.hip) compile for gfx950 without scratch, and the LDS-resident ones - two 64 x 65 matrices of
doubles - stay within what one workgroup can have."""
import re
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_kernel_resources import HIPCC, ROOT, SRC, _pick, _resources  # noqa: E402

KERNELS = ("k_eig_small", "k_eig_check", "k_eig_colsum", "k_eig_prep", "k_eig_gram", "k_eig_rot", "k_eig_apply", "k_eig_rayleigh", "k_eig_rank", "k_eig_emit")
LDS_PER_WORKGROUP = 160 * 1024  # gfx950: 160 KiB of LDS per CU, all of it addressable by one workgroup


def test_eig_kernels_use_no_scratch():
    res = _resources("eig.hip")
    eig = _pick(res, "k_eig_")
    for name in KERNELS:
        assert any(name in k for k in eig), name
    spilled = {k: v["scratch"] for k, v in eig.items() if v["scratch"] != 0}
    assert not spilled, spilled
    # the solver and the update hold 4 x 4 register tiles beside their state: two workgroups per CU need <= 256 registers
    for key in ("k_eig_rot", "k_eig_apply", "k_eig_small"):
        for name, r in _pick(res, key).items():
            assert r["vgpr"] + r["agpr"] <= 256, (name, r)


def test_lds_resident_kernels_fit_their_workgroup():
    _resources("eig.hip")  # skips without hipcc
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fvisibility=hidden", f"-I{ROOT / 'include'}",
           "-S", "--cuda-device-only", str(SRC / "eig.hip"), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=SRC)
    assert r.returncode == 0, r.stderr[-2000:]
    lds = {m.group(1): int(m.group(2)) for m in re.finditer(r"Function Name: (\S+).*?LDS Size \[bytes/block\]: (\d+)", r.stderr, re.S)}
    matrices = 2 * 64 * 65 * 8  # S and U; the sort's ranks and the control words come on top
    for needle in ("k_eig_small", "k_eig_rot", "k_eig_apply"):
        hits = {k: v for k, v in lds.items() if needle in k}
        assert hits, needle
        for name, size in hits.items():
            assert matrices < size <= matrices + 1024 and size <= LDS_PER_WORKGROUP // 2, (name, size)  # two workgroups per CU
    for name, size in lds.items():
        if "k_eig_gram" in name:
            assert size == 64 * 65 * 8, (name, size)  # one staged chunk
        elif not any(k in name for k in ("k_eig_small", "k_eig_rot", "k_eig_apply")):
            assert size <= 64, (name, size)
