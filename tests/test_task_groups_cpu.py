"""The rule by which k_task_groups cuts the tasks of one window and congruence class into the groups of k_hscan_same (bsx_groups.h: bsx_group_cut), driven on
the host by tests/harness/groups_check.cpp over random and directed runs: sizes 1, 2, 63, 64, 65, 127, 128, 129 and 1 024, caps 1, 16 and 64, D = 0, 1, 2, offsets
from one to five classes of h >> 5, negative ones among them.  Every task is in exactly one group of 1 .. Rg members that lie within 32 D of the group's frame and
are congruent to it, rows sorted by d with d = 0 in row 0; a run that one frame holds gives ceil(N / Rg) groups whose sizes differ by one at most (70 -> 35 + 35,
65 -> 33 + 32) and none of one task; the function returns within N turns."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_group_cut_rule(tmp_path):
    exe = str(tmp_path / "groups_check")
    subprocess.check_call([HIPCC, "-O1", "-o", exe, os.path.join(ROOT, "tests", "harness", "groups_check.cpp")], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
