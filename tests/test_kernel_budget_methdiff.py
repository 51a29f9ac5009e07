"""Register / scratch budget of the two-sample kernels of bsx_meth.hip, screened as tests/test_kernel_budget.py screens the aligner's:
hipcc cross-compiles gfx950 and reports the resource usage.  All of them run at eight waves per SIMD (64 VGPRs or fewer) without scratch: k_meth_fisher is a
thread per row whose lanes walk supports of different lengths, so it lives on the other waves of its SIMD; the compaction passes and the interval kernel
wait for memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "bsmap_amd", "csrc", "bsx_meth.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# kernel (mangled-name fragment) -> (max VGPRs, max scratch bytes per lane); today 20, 38, 38, 56, 56
BUDGET = {
    "12k_diff_countE": (64, 0),
    "11k_diff_emitE": (64, 0),
    "13k_meth_fisherE": (64, 0),
    "19k_meth_diff_regionsILi4EE": (64, 0),
    "19k_meth_diff_regionsILi16EE": (64, 0),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_diff_kernels_stay_within_their_register_budget(tmp_path):
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
