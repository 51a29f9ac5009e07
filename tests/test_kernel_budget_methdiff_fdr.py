"""Register / scratch budget of the q-value and DMR kernels of bsx_meth.hip, screened as tests/test_kernel_budget_methdiff.py screens the
two-sample kernels: hipcc cross-compiles gfx950 and reports the resource usage.  All of them are a few loads and stores per item and wait for memory, so
the cap is the first occupancy step at or above what they use: eight waves per SIMD (64 VGPRs or fewer), without scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "bsmap_amd", "csrc", "bsx_meth.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel (mangled-name fragment) -> (max VGPRs, max scratch bytes per lane); today 10, 14, 6, 16, 28, 8, 26, 16 VGPRs
BUDGET = {
    "9k_bh_keysE": (64, 0),
    "10k_bh_ratioE": (64, 0),
    "12k_bh_scatterE": (64, 0),
    "12k_cand_countE": (64, 0),
    "11k_cand_emitE": (64, 0),
    "12k_head_countE": (64, 0),
    "11k_head_emitE": (64, 0),
    "10k_dmr_runsE": (64, 0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_fdr_kernels_stay_within_their_register_budget(tmp_path):
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                          "-c", SRC, "-o", str(tmp_path / "a.o")], capture_output=True, text=True, timeout=1200, cwd=os.path.dirname(SRC))
    assert res.returncode == 0, res.stderr[-2000:]
    usage, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1).split()[0]] = int(m.group(2))
    for frag, (vg, sc) in BUDGET.items():
        hits = [u for n, u in usage.items() if frag in n]
        assert len(hits) == 1, (frag, list(usage))
        assert hits[0]["VGPRs"] <= vg and hits[0]["ScratchSize"] <= sc, (frag, hits[0], "budget", vg, sc)
