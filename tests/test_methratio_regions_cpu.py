"""Pooled methylation per interval and per bin (methratio --regions / --region-out, -w / -b), the parts that need no GPU: the model of
regions_model.py on cases computed by hand, the option surface of bsmap_amd.methratio, and the rule by which bsx_meth_regions cuts an
interval into tiles (bsmap_amd/csrc/bsx_meth_tiles.h through tests/harness/tiles_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import ctsnp_model as M
import regions_model as R
from conftest import HOST_SAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _six():
    """ACGTCA: C at 1 (CG), G at 2 (CG), C at 4 (its second neighbour is outside the chromosome: class 3)"""
    K = M.Counters(["ACGTCA"])
    K.depth[0] = [0, 4, 2, 0, 3, 0]
    K.meth[0] = [0, 1, 2, 0, 0, 0]
    return K


def test_six_letters_three_sites():
    K = _six()
    S = R.site_table(K, 1, 0, 0)
    assert S[0] == [None, (1, 1, 4, 4 << 16, 1 << 16), (1, 2, 2, 2 << 16, 2 << 16), None, (1, 0, 3, 3 << 16, 0), None]
    assert R.interval_sums(S, 0, 0, 6) == [3, 3, 9, 9 << 16, 3 << 16]
    assert R.interval_sums(S, 0, 2, 5) == [2, 2, 5, 5 << 16, 2 << 16]
    assert R.interval_sums(S, 0, 0, 1) == R.interval_sums(S, 0, 3, 3) == R.interval_sums(S, 0, 9, 12) == [0] * 5
    assert R.interval_sums(S, 0, 4, 1000) == [1, 0, 3, 3 << 16, 0]                      # end clipped; a covered C without a methylated read counts
    assert R.bin_sums(S, 0, 4) == [[2, 3, 6, 6 << 16, 3 << 16], [1, 0, 3, 3 << 16, 0]]
    assert R.bin_sums(S, 0, 6) == [[3, 3, 9, 9 << 16, 3 << 16], [0] * 5]                # len // B + 1 bins: the last one is empty here
    assert R.bin_sums(S, 0, 1)[1:3] == [[1, 1, 4, 4 << 16, 1 << 16], [1, 2, 2, 2 << 16, 2 << 16]] and len(R.bin_sums(S, 0, 1)) == 7
    assert len(R.bin_sums(S, 0, 1 << 31)) == 1
    assert R.interval_sums(R.site_table(K, 3, 0, 0), 0, 0, 6) == [2, 1, 7, 7 << 16, 1 << 16]   # min_depth 3 drops the G
    assert R.interval_sums(R.site_table(K, 1, 0, 1), 0, 0, 6) == [2, 3, 6, 6 << 16, 3 << 16]   # CG only: the C at 4 is in no CG
    assert R.interval_sums(R.site_table(K, 0, 0, 0), 0, 0, 6) == [3, 3, 9, 9 << 16, 3 << 16]   # min_depth 0 adds no site
    assert R.wig_text(["x"], S, 4) == "track type=wiggle_0\nvariableStep chrom=x span=4\n1\t0.500\n5\t0.000\n"
    assert R.wig_text(["x"], R.site_table(K, 5, 0, 0), 4) == "track type=wiggle_0\nvariableStep chrom=x span=4\n"
    # the whole chromosome as one region: the table's own row for depth 9, 3 methylated
    assert R.region_text(["x"], S, [(0, 0, 6, "all"), (0, 3, 3, ".")]) == (
        R.REGION_HEADER + "x\t0\t6\tall\t3\t3\t9\t9.00\t0.333\t" + "\t".join(M.row_fields(9, 3, 0, 0, 0).split("\t")[3:]) + "\nx\t3\t3\t.\t0\t0\t0\t0.00\tNA\tNA\tNA\n")


def test_ct_snp_site():
    """g = 1, ga = 3, d = 5, m = 4: e = rint(5/3 * 65536) = rint(109226.67) = 109227, and the four methylated reads are clipped to it"""
    K = M.Counters(["AACAA"])
    K.depth[0][2], K.meth[0][2], K.rev_g[0][2], K.rev_ga[0][2] = 5, 4, 1, 3
    assert R.site(K, 0, 2, 1, 1, 0) == (1, 4, 5, 109227, 109227)
    assert R.site(K, 0, 2, 1, 0, 0) == (1, 4, 5, 5 << 16, 4 << 16)       # mode off: the raw depth
    assert R.site(K, 0, 2, 1, 2, 0) is None                               # skip mode: g != ga
    S = R.site_table(K, 1, 1, 0)
    assert R.interval_sums(S, 0, 0, 5) == [1, 4, 5, 109227, 109227]
    assert R.region_fields([1, 4, 5, 109227, 109227]).startswith("1\t4\t5\t1.67\t1.000\t")
    K.meth[0][2] = 1                                                      # below the effective depth: no clip
    assert R.site(K, 0, 2, 1, 1, 0) == (1, 1, 5, 109227, 65536)
    K.rev_g[0][2] = 0                                                     # every opposite-strand call converted: no site under `correct`
    assert R.site(K, 0, 2, 1, 1, 0) is None
    K.rev_g[0][2] = K.rev_ga[0][2] = 3
    assert R.site(K, 0, 2, 1, 1, 0) == (1, 1, 5, 5 << 16, 1 << 16)
    K.depth[0][2], K.rev_g[0][2], K.rev_ga[0][2] = 1, 1, 1 << 17          # a tie: 0.5 rounds to the even 0; such a region has no ratio
    assert R.site(K, 0, 2, 1, 1, 0) == (1, 1, 1, 0, 0)
    assert R.region_fields([1, 1, 1, 0, 0]) == "1\t1\t1\t0.00\tNA\tNA\tNA"


def test_bed_model():
    names, lens = ["a", "b"], [100, 7]
    text = "#c\ntrack x\nbrowser y\n\na\t5\t9\tlab\textra\r\nb 0   900\nzz\t1\t2\n \t \na\t200\t300\nb\t7\t7"
    assert R.parse_bed(text, names, lens) == ([(0, 5, 9, "lab"), (1, 0, 7, "."), (0, 100, 100, "."), (1, 7, 7, ".")], 1)
    assert R.parse_bed("", names, lens) == ([], 0) and R.parse_bed("\n\n", names, lens) == ([], 0)
    for bad in ("a\t5", "a\t9\t5", "a\t-1\t5", "a\t1\t5x", "a\t1\t" + "9" * 30, "zz\t3\t2", "a\t\t5\t9"[:5]):
        assert R.parse_bed("a\t1\t2\n\n" + bad + "\na\t1\t2\n", names, lens) == 3, bad


def test_parser_options_and_defaults():
    from bsmap_amd import methratio
    ap = methratio.build_parser()
    o = ap.parse_args(["-o", "t", "-d", "g.fa", "in.bsp"])
    assert (o.wig, o.wig_bin, o.regions, o.region_out) == (None, 25, None, None)
    o = ap.parse_args(["-o", "t", "-d", "g.fa", "-w", "t.wig", "-b", "50", "--regions", "r.bed", "--region-out", "r.txt", "in.bsp"])
    assert (o.wig, o.wig_bin, o.regions, o.region_out) == ("t.wig", 50, "r.bed", "r.txt")
    o = ap.parse_args(["-o", "t", "-d", "g.fa", "--wig", "t.wig", "--wig-bin", "1", "in.bsp"])
    assert (o.wig, o.wig_bin) == ("t.wig", 1)
    with pytest.raises(SystemExit):
        ap.parse_args(["-o", "t", "-d", "g.fa", "-b", "0", "in.bsp"])
    assert "BSMAP" in methratio.__doc__ and "--wig" in methratio.__doc__ and "--regions" in methratio.__doc__


@pytest.mark.parametrize("kw", [dict(wig="t.wig", wig_bin=0), dict(wig_bin=-3), dict(regions="r.bed"), dict(region_out="r.txt")])
def test_run_refuses_before_the_library_is_touched(kw, tmp_path, monkeypatch):
    from bsmap_amd import methratio
    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(methratio, "_bind", no_library)
    with pytest.raises(ValueError):
        methratio.run(str(tmp_path / "absent.fa"), [str(tmp_path / "absent.bsp")], str(tmp_path / "t.txt"), **kw)
    assert not os.listdir(tmp_path)


# ---- the tile-cutting rule ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tiles") / "tiles_check")
    subprocess.run(["g++"] + HOST_SAN_FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "harness", "tiles_check.cpp")], check=True)
    def run(*lens):
        r = subprocess.run([exe] + [str(x) for x in lens], capture_output=True, timeout=120)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
        return r.stdout.decode().split("\n")[:-1]
    return run


def test_tile_cutting_rule(tiles):
    T = int(tiles()[0].split()[1])
    assert 64 <= T <= 8192 and T % 64 == 0   # a few thousand at the most: whole strides of a wave
    lens = [0, 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 63, 100 * T + 5]
    out = tiles(*lens)
    assert out[0] == "tile %d" % T
    at = 1
    for k, n in enumerate(lens):
        iv = 7 + k
        head = out[at].split()
        ntile = int(head[5])
        assert head[:4] == ["interval", str(iv), "len", str(n)] and int(head[7]) == ntile == (n + T - 1) // T
        got = [tuple(int(x) for x in l.split()) for l in out[at + 1:at + 1 + ntile]]
        at += 1 + ntile
        assert all(g[0] == iv for g in got)
        pos = 0
        for _, off, ln, single in got:       # disjoint and covering: every tile starts where the one before it ended
            assert off == pos and 1 <= ln <= T
            pos += ln
            assert single == (1 if ntile == 1 else 0)
        assert pos == n
    assert at == len(out)


# ---- the launches of a call and their block width --------------------------------------------------------------------------------------
def launch_lists(T):
    """directed lists of interval lengths (in positions), then seeded ones: empty intervals in runs, single tiles, intervals of more tiles than any chunk"""
    directed = [[], [0], [1], [0, 0, 0], [9 * T], [9 * T, 9 * T], [T] * 17, [0] * 17, [1, 9 * T, 1],
                [0, T, 0, 0, 5 * T, 0, 0, 0, T + 1, 0],                        # empty ones at the first and last place of a launch, and alone
                [T, T, 0, 0, 0, 0, 0, 0, 0, 0, 0, T, T, 0], [0, 0, 2 * T, 0, 0, 3 * T + 1, 0, 0, 0, 0, 0, 4 * T, 4 * T + 1],
                [2 * T, 3 * T, T, 0, 8 * T, 8 * T + 1, 7 * T, 1, 1, 1, 1, 1, 1, 1, 1, 1, 40 * T]]
    rng = np.random.default_rng(11)
    seeded = []
    for n in (1, 2, 3, 7, 8, 9, 40, 200):
        for _ in range(3):
            kind = rng.integers(0, 4, n)   # 0: empty, 1: one tile, 2: a few tiles, 3: more than 8
            tiles = np.where(kind == 0, 0, np.where(kind == 1, 1, np.where(kind == 2, rng.integers(2, 6, n), rng.integers(9, 30, n))))
            seeded.append([int(t) * T - (int(rng.integers(0, T)) if t else 0) for t in tiles])
    return directed, seeded


def model_launches(ntiles, chunk):
    """the rule restated: a launch takes intervals while it holds fewer than `chunk` of them and fewer than `chunk` tiles"""
    cuts, a = [0], 0
    while a < len(ntiles):
        b, nt = a, 0
        while b < len(ntiles) and b - a < chunk and nt < chunk:
            nt += ntiles[b]
            b += 1
        cuts.append(b)
        a = b
    return cuts


@pytest.mark.parametrize("chunk", [1, 2, 5, 8])
def test_launch_cut_rule(tiles, chunk):
    T = int(tiles()[0].split()[1])
    directed, seeded = launch_lists(T)
    seen = set()
    for lens in directed + seeded:
        ntiles = [(n + T - 1) // T for n in lens]
        out = tiles("launches", chunk, *lens)
        assert len(out) == 1 and out[0].split()[0] == "launches"
        cuts = [int(x) for x in out[0].split()[1:]]
        assert cuts[0] == 0 and cuts[-1] == len(lens) and all(x < y for x, y in zip(cuts, cuts[1:])), (lens, cuts)   # a partition of [0, n) in order, none empty
        assert cuts == model_launches(ntiles, chunk), lens
        for a, b in zip(cuts, cuts[1:]):
            assert b - a <= chunk and sum(ntiles[a:b - 1]) < chunk, (lens, a, b)
            if b < len(lens):                                     # a launch ends early only where it is full
                assert b - a == chunk or sum(ntiles[a:b]) >= chunk, (lens, a, b)
            if ntiles[b - 1] > chunk:
                seen.add("alone" if b - a == 1 else "last")       # an interval of more tiles than the chunk is placed
            if b - a > 1 and any(ntiles[a:b]):
                seen |= {"empty first"} if not ntiles[a] else set()
                seen |= {"empty last"} if not ntiles[b - 1] else set()
            if not any(ntiles[a:b]):
                seen.add("all empty")
        assert all(t <= chunk or any(b - 1 == i for b in cuts[1:]) for i, t in enumerate(ntiles)), lens   # .. as its launch's last interval
    assert seen >= ({"alone", "all empty"} if chunk == 1 else {"alone", "last", "empty first", "empty last", "all empty"}), seen


def test_wide_rule(tiles):
    T = int(tiles()[0].split()[1])
    wide = lambda *lens: tiles("wide", *lens) == ["wide 1"]
    narrow = lambda *lens: tiles("wide", *lens) == ["wide 0"]
    assert narrow() and narrow(0) and narrow(1) and narrow(T, T, T)
    assert narrow(63 * T) and narrow(62 * T + 1) and wide(63 * T + 1) and wide(64 * T) and wide(200 * T + 5)   # 63 tiles against 64
    assert narrow(*[63 * T] * 10) and wide(*[64 * T] * 10)
    assert narrow(64 * T, *[1] * 64) and wide(64 * T, *[1] * 63) and narrow(64 * T, *[1] * 65)                   # exactly half is not wide
    assert wide(64 * T + 1, *[T] * 64) and narrow(64 * T + 1, *[T] * 65)                                         # 65 of 129: one tile over half
    assert narrow(64 * T, 32 * T, 32 * T) and wide(64 * T, 32 * T, 31 * T) and wide(64 * T, 0, 0, 63 * T, 0)     # shorter intervals of many tiles count as short
    assert wide(0, 64 * T, 0) and wide(32 * T, 64 * T, 31 * T + 1, 65 * T) and narrow(*[63 * T, 64 * T] * 3, T, T, T)
