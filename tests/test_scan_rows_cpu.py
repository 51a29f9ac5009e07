"""The LDS row of k_hscan_same's groups of 129-160 nt reads in the order of evaluation (bsx_rows.h), driven on the host by tests/harness/rows_check.cpp: random and
directed reads — planes, thresholds 0, 2, 6, 15 and the largest, offset classes 0-2, an N at either end of every word, a last word of 1, 16, 31 and 32 letters —
are packed and read back half by half (the second half poisoned while the first two evaluated words, the threshold, the plain flag and the class are read), and the
per-word mismatch counts in the order 0, 4, 3, 2, 1, formed as the kernel forms them, must be those of bsx_plane_mismatch and bsx_plane_mismatch_full on the
unpacked planes.  The host model of the ways a read leaves the four chunks of a step (chunk-major, joint with the chunks that are not alive skipped, joint with
them evaluated and ignored, and the shipped form: one test per word on the smallest of a lane's four counts where every lane holds a candidate) keeps in every form
exactly the candidates within the threshold over all five words; the skipping joint form takes the words of the chunk-major form, the ignoring one at least as
many, and the shipped form exactly the ignoring one's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_rows_in_evaluation_order_and_the_exit_model(tmp_path):
    exe = str(tmp_path / "rows_check")
    subprocess.check_call([HIPCC, "-O1", "-o", exe, os.path.join(ROOT, "tests", "harness", "rows_check.cpp")], stderr=subprocess.DEVNULL)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
