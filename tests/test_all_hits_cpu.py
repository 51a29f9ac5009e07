"""All hits (include/bsx.h: bsx_batch_set_all_hits; the command line's --all-hits=FILE), the parts that need no GPU: the four calls are declared,
exported and bound; bsx_span is the 16-byte record the device writes; the command line lists the option and refuses it with -r 0 before it looks
for a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bsmap_amd as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "bsx.h")
EXE = os.path.join(ROOT, "bsmap_amd", "bsmap")
CALLS = ["bsx_batch_set_all_hits", "bsx_batch_all_hits_need", "bsx_batch_all_hits_spans", "bsx_batch_all_hits_fetch"]


@pytest.fixture(scope="module")
def L():
    B.build()
    return B.lib()


def test_calls_are_declared_exported_and_bound(L):
    hdr = open(HDR).read()
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/bsx.h"
        assert name in B.EXPORTS
        assert getattr(L, name).argtypes is not None, f"{name} has no ctypes signature"
    for m in ("set_all_hits", "all_hits", "all_hits_need"):
        assert callable(getattr(B._Batch, m))
    assert callable(B.all_hits_lists)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_span_is_16_bytes_in_c_and_in_numpy(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bsx.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %d\\n", sizeof(bsx_span), offsetof(bsx_span, off), offsetof(bsx_span, n), offsetof(bsx_span, n_fwd), '
                   'BSX_SPAN_DROPPED == 0xFFFFFFFFFFFFFFFFull); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()
    assert out == ["16", "0", "8", "12", "1"]
    d = B.SPAN_DTYPE
    assert d.itemsize == 16 and [d.fields[f][1] for f in ("off", "n", "n_fwd")] == [0, 8, 12] and B.SPAN_DROPPED == 2 ** 64 - 1


def test_lists_from_spans():
    """the helper that turns one unit's spans into the lists debug_hits / debug_pairs return"""
    pool = np.array([7, 7, 2, 10, 3, 20, 0 | (1 << 16) | (2 << 24), 0xFFFFFFFF & -5, 4, 30, 5, 40], np.uint32)
    sp = np.zeros(3, B.SPAN_DTYPE)
    sp[0] = (2, 2, 1)
    sp[2] = (6, 1, 0)
    assert B.all_hits_lists(sp, pool) == ([(2, 10), (3, 20)], [], [(0, 1, 2, -5, 4, 30, 5, 40)])
    sp[1] = (B.SPAN_DROPPED, 3, 2)
    assert B.all_hits_lists(sp, pool)[1] is None


def _run(args, cwd):
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=dict(os.environ, BSX_PIN="0"), timeout=120)


def test_command_line_lists_the_option(L, tmp_path):
    r = _run(["-h"], str(tmp_path))
    assert "--all-hits=FILE" in r.stdout


def test_command_line_refuses_all_hits_with_r0_before_any_device_work(L, tmp_path):
    (tmp_path / "g.fa").write_text(">c\n" + "ACGTTGCA" * 200 + "\n")
    (tmp_path / "a.fq").write_text("@r\n" + "ACGTTGCA" * 8 + "\n+\n" + "I" * 64 + "\n")
    side = tmp_path / "x.tsv"
    r = _run([f"--all-hits={side}", "-r", "0", "-a", "a.fq", "-d", "g.fa", "-o", "o.sam"], str(tmp_path))
    txt = r.stdout + r.stderr
    assert r.returncode == 1 and "--all-hits needs -r 1" in r.stderr, (r.returncode, txt[-400:])
    assert "device" not in txt.lower() and not side.exists() and not (tmp_path / "o.sam").exists()
    # -r 0 given first, or a missing file name, are caught the same way
    r = _run(["-r", "0", f"--all-hits={side}", "-a", "a.fq", "-d", "g.fa", "-o", "o.sam"], str(tmp_path))
    assert r.returncode == 1 and "--all-hits needs -r 1" in r.stderr
    r = _run(["--all-hits=", "-a", "a.fq", "-d", "g.fa", "-o", "o.sam"], str(tmp_path))
    assert r.returncode != 0 and "unknown option" in r.stdout
