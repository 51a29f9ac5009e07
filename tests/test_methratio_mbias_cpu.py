"""The surface of the M-bias / cycle-trim feature of bsmap_amd.methratio that needs no GPU: the four C calls are declared in
include/bsx.h, exported by libbsx.so and bound by methratio._bind(); the command line takes --mbias / --trim-5p / --trim-3p and refuses
negative trims; the header's BSX_MBIAS_CYCLES is the constant the Python side shapes its fetch buffer with."""
import os
import re

import pytest

import bsmap_amd as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsx_meth_set_cycle_trim", "bsx_meth_set_mbias", "bsx_meth_mbias_fetch", "bsx_meth_write_mbias")
HEADER = open(os.path.join(ROOT, "include", "bsx.h")).read()


@pytest.fixture(scope="module")
def L():
    B.build()
    return B.lib()


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(L, name):
    from bsmap_amd import methratio
    assert re.search(r"\bint\s+%s\s*\(\s*bsx_meth\s*\*" % name, HEADER), f"{name} is not declared in include/bsx.h"
    assert name in B.EXPORTS
    assert hasattr(L, name), f"{name} is not exported by libbsx.so"
    assert getattr(methratio._bind(), name).argtypes, f"{name} is not bound by methratio._bind()"


def test_cycle_count_of_header_and_python_agree():
    from bsmap_amd import methratio
    m = re.search(r"^#define\s+BSX_MBIAS_CYCLES\s+(\d+)\s*$", HEADER, re.M)
    assert m and int(m.group(1)) == methratio.MBIAS_CYCLES == 1024




def parsed(monkeypatch, argv):
    """the keyword arguments main() hands to run() for this command line"""
    from bsmap_amd import methratio
    seen = {}

    def fake_run(reffile, infiles, outfile, **kw):
        seen.update(kw, reffile=reffile, infiles=infiles, outfile=outfile)
        return ""
    monkeypatch.setattr(methratio, "run", fake_run)
    methratio.main(argv)
    return seen


def test_options_are_accepted(monkeypatch):
    kw = parsed(monkeypatch, ["-o", "t.txt", "-d", "g.fa", "--mbias", "m.tsv", "--trim-5p", "3", "--trim-3p=7", "a.bsp"])
    assert (kw["mbias"], kw["trim5"], kw["trim3"], kw["infiles"]) == ("m.tsv", 3, 7, ["a.bsp"])
    kw = parsed(monkeypatch, ["-o", "t.txt", "-d", "g.fa", "--mbias=m2.tsv", "a.sam"])
    assert (kw["mbias"], kw["trim5"], kw["trim3"]) == ("m2.tsv", 0, 0)
    kw = parsed(monkeypatch, ["-o", "t.txt", "-d", "g.fa", "a.sam"])
    assert (kw["mbias"], kw["trim5"], kw["trim3"], kw["trim_fillin"]) == (None, 0, 0, 2)


@pytest.mark.parametrize("opt", ["--trim-5p", "--trim-3p"])
def test_negative_trims_are_an_argparse_error(monkeypatch, capsys, opt):
    with pytest.raises(SystemExit) as e:
        parsed(monkeypatch, ["-o", "t.txt", "-d", "g.fa", opt + "=-1", "a.bsp"])
    assert e.value.code == 2 and opt in capsys.readouterr().err


def test_run_takes_the_new_arguments_with_their_defaults():
    import inspect
    from bsmap_amd import methratio
    p = inspect.signature(methratio.run).parameters
    assert (p["mbias"].default, p["trim5"].default, p["trim3"].default) == (None, 0, 0)
