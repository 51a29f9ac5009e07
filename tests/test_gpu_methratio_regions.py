"""Pooled methylation per interval and per bin of bsmap_amd.methratio (bsx_meth_regions / _bins / _write_regions / _write_wig, --regions /
--region-out, -w / -b) against the pure-Python model of regions_model.py, which never looks at the library's output.

The v2.6 script the project mirrors has neither option: the model is the yardstick, and the tests of part 3 tie the sums to code that is
pinned to the reference (bsx_meth_report_chr, the v2.6 tables of tests/golden/methratio.json.gz)."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

from bsmap_amd import _check

import ctsnp_model as M
import golden_util as G
import meth_util as U
import regions_model as R

pytestmark = pytest.mark.gpu
STRANDS = M.STRANDS
BSX_ERR_ARG, BSX_ERR_IO = -1, -2
MODES, MASKS, DEPTHS = (0, 1, 2), (0, 1, 6), (1, 3)          # off / correct / skip; no filter / CG / CHG|CHH
GRID = [(mode, mask, md, cpg) for mode in MODES for mask in MASKS for md in DEPTHS for cpg in (0, 1)]
GRID_IDS = ["%s-mask%d-m%d%s" % (M.MODES[mode], mask, md, "-g" if cpg else "") for mode, mask, md, cpg in GRID]


def _lib():
    from bsmap_amd import methratio
    return methratio._bind()


POISON = 0xA5A5A5A5A5A5A5A5   # what the sums hold before the call: a cell the library leaves out shows


def handle(fa, snp=False):
    return U.open_meth(fa, snp=1 if snp else 0)


def rule(h, mode, mask):
    """mode: 0 stays off (a handle without the rev cells), 1 <-> 2 at any time"""
    if mode:
        h.set_ct_snp(mode)
    h.set_contexts(mask)


def got_bins(h, c, B, min_depth):
    """the raw call into a preset array, and Meth.bins, which has to give the same"""
    n, n2 = C.c_uint64(), C.c_uint64()
    assert h.L.bsx_meth_bins(h.h, c, B, min_depth, 0, None, C.byref(n)) == BSX_ERR_ARG   # the size query
    out = np.full((n.value, 5), POISON, np.uint64)
    _check(h.L.bsx_meth_bins(h.h, c, B, min_depth, n.value, out.ctypes.data, C.byref(n2)))
    assert n2.value == n.value and np.array_equal(h.bins(c, B, min_depth), out)
    return out.tolist()


def got_regions(h, ivs, min_depth):
    """ivs: [(chr id, start, end)] -> [[N, M, D, E, MC]], likewise"""
    a = [np.array([iv[k] for iv in ivs], np.uint32) for k in range(3)]
    out = np.full((len(ivs), 5), POISON, np.uint64)
    _check(h.L.bsx_meth_regions(h.h, len(ivs), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, min_depth, out.ctypes.data))
    assert np.array_equal(h.regions(*a, min_depth), out)
    return out.tolist()


def got_wig(h, path, B, min_depth):
    h.write_wig(path, B, min_depth)
    return open(path, "rb").read()


def got_region_file(h, bed, path, min_depth):
    nw, nd = h.write_regions(bed, path, min_depth)
    return open(path, "rb").read(), nw, nd


def got_report(h, c, min_depth, meth0=1):
    pos, dep, met, cov, sd = h.report(c, min_depth, meth0)
    return list(zip(pos.tolist(), met.tolist(), dep.tolist())), cov, sd


def got_table(h, path, min_depth=1, meth0=1):
    text, nc, nd = U.written_table(h, path, min_depth, meth0)
    return text.encode(), nc, nd


def make_read(rng, ref, snp, pos, L, st, noise=True):
    """the reference letters under the read with bisulfite-like conversion on the read's own strand, planted C/T SNPs shown by the other one, and noise
    (as the edge set of test_gpu_methratio_ctsnp.py makes its reads)"""
    out = []
    match, convert, rc_match, rc_convert = ("C", "T", "G", "A") if st % 2 == 0 else ("G", "A", "C", "T")
    for g in range(pos, pos + L):
        x, r = ref[g], rng.random()
        if x == match and r < 0.5:
            x = convert
        elif x == rc_match and g in snp and rng.random() < snp[g]:
            x = rc_convert
        elif noise and r > 0.96:
            x = "ACGTN"[int(rng.integers(0, 5))]
        out.append(x)
    return "".join(out)


class World:
    """Four chromosomes of 1, 5, 4 099 and 2 T + 67 letters (T = bsx_meth_region_tile()), named so that the sorted order is not the id order; random ACGT
    with CG runs planted at both ends; about 20 000 alignments of 30-60 nt on all four strands, all but one in 25 of them on the first two fifths of their
    chromosome (the rest of it is covered thinly: -m 3 drops sites there), short reads on the two tiny chromosomes; C/T SNPs planted as in the §3.8 edge set."""
    SEED, N_ALN, TRIM = 47, 20000, 2

    def __init__(self, T):
        rng = np.random.default_rng(self.SEED)
        self.T = T
        self.names = ["wd_one", "wc_five", "wb_mid", "wa_long"]
        self.refs = ["C", "CGCGC"]
        for n in (4099, 2 * T + 67):
            s = rng.choice(list("ACGT"), n).tolist()
            s[:8], s[-8:] = list("CGCGCGCG"), list("CGCGCGCG")
            self.refs.append("".join(s))
        self.lens = [len(r) for r in self.refs]
        self.fasta = "".join(">%s\n%s" % (n, "".join(s[i:i + 60] + "\n" for i in range(0, len(s), 60))) for n, s in zip(self.names, self.refs))
        self.snp = []
        for ref in self.refs:
            cg = [i for i, ch in enumerate(ref) if ch in "CG"]
            p = {i: 0.5 for i in cg if rng.random() < 0.05}
            if len(cg) > 20:
                p.update({int(i): 1.0 for i in rng.choice(cg, 6, replace=False)})
            self.snp.append(p)
        alns = []
        for k in range(self.N_ALN):
            c = 2 + (k % 3 != 0)                       # two in three on the long chromosome
            L = int(rng.integers(30, 61))
            n = self.lens[c]
            if k % 50 == 0:
                pos = (0, n - L)[(k // 50) % 2]         # flush with either end
            elif k % 25 == 0:
                pos = int(rng.integers(0, n - L + 1))
            else:
                pos = int(rng.integers(0, 2 * n // 5))
            st = int(rng.integers(0, 4))
            alns.append((c, pos, st, 0, -1, make_read(rng, self.refs[c], self.snp[c], pos, L, st)))
        for k in range(40):                             # the tiny chromosomes: '++' and '-+' reads (no fill-in to trim off)
            alns.append((0, 0, k % 2, 0, -1, "CT"[k % 3 == 0]))
            L = 1 + k % 5
            pos = k % (6 - L)
            alns.append((1, pos, k % 2, 0, -1, make_read(rng, self.refs[1], self.snp[1], pos, L, k % 2, noise=False)))
        self.alns = [alns[i] for i in rng.permutation(len(alns)).tolist()]
        K = M.pileup(self.refs, self.alns, self.TRIM)
        self.K = {0: K, 1: M.combine_cpg(K)}
        self._S, self._h = {}, {}

    def S(self, mode, mask, md, cpg):
        key = (mode, mask, md, cpg)
        if key not in self._S:
            self._S[key] = R.site_table(self.K[cpg], md, mode, mask)
        return self._S[key]

    def handle(self, mode, mask, cpg):
        """one pile-up per (SNP cells or not, folded or not), shared by all tests: the calls under test change no counter"""
        key = (bool(mode), cpg)
        if key not in self._h:
            h = handle(self.fa, snp=bool(mode))
            h.add(self.alns, self.TRIM)
            if cpg:
                h.combine_cpg()
            self._h[key] = h
        rule(self._h[key], mode, mask)
        return self._h[key]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    w = World(_lib().bsx_meth_region_tile())
    w.dir = tmp_path_factory.mktemp("regions_world")
    w.fa = str(w.dir / "world.fa")
    open(w.fa, "w").write(w.fasta)
    yield w
    for h in w._h.values():
        h.close()


def intervals(w):
    """(chr id, start, end, label) of test 2, end as given (one of them beyond the chromosome)"""
    T, A, B_ = w.T, 2, 3
    nA, nB = w.lens[A], w.lens[B_]
    out = []
    for k, ln in enumerate((0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1)):
        out.append((B_, 3 + k, 3 + k + ln, "len%d" % ln))
        if ln <= nA:
            out.append((A, 0, ln, "A_from0_%d" % ln))            # starts at 0
            out.append((A, nA - ln, nA, "A_to_end_%d" % ln))     # ends at the chromosome's last letter
        out.append((B_, nB - min(ln, nB), nB, "B_to_end_%d" % ln))
    out += [(B_, 0, nB, "whole_long"), (A, 0, nA, "whole_mid"), (B_, nB - 100, nB + 500, "clipped"), (A, nA + 5, nA + 9, "beyond"),
            (0, 0, 1, "one"), (0, 0, 0, "one_empty"), (1, 0, 5, "five"), (1, 1, 4, "five_inner"), (1, 4, 5, "five_last")]
    out += [(B_, 100, 1100, "ov1"), (B_, 600, 1600, "ov2"), (B_, 600, 601, "ov3"), (A, T - 10, T + 10, "ov4"), (A, T, T + 1, "ov5")]
    out += [(B_, 1000, 1000 + T + 5, "same")] * 4
    out += sorted(out, key=lambda r: (r[0], r[1], r[2]), reverse=True)   # the whole list again, descending
    return out


def bed_text(w, ivs):
    return "".join("%s\t%d\t%d\t%s\n" % (w.names[c], a, b, lab) for c, a, b, lab in ivs)


def test_world_covers_what_it_claims(world):
    """the generated set holds what the other tests rely on (the model's side only; no library call)"""
    K = world.K[0]
    S0, S3 = world.S(0, 0, 1, 0), world.S(0, 0, 3, 0)
    for c in range(4):
        assert any(S0[c]), c                                                       # every chromosome has a site
    assert world.T <= 8192 and world.lens == [1, 5, 4099, 2 * world.T + 67]
    n0, n3 = (sum(1 for c in range(4) for v in S[c] if v) for S in (S0, S3))
    assert n3 < n0 - 200                                                           # -m 3 matters
    S1, S2 = world.S(1, 0, 1, 0), world.S(2, 0, 1, 0)
    corrected = [v for c in range(4) for v in S1[c] if v and v[3] != v[2] << 16]
    assert len(corrected) > 50 and any(v[4] < v[1] << 16 for v in corrected)     # effective depths, and the clip of the methylated count
    assert sum(1 for c in range(4) for v in S2[c] if v) < sum(1 for c in range(4) for v in S1[c] if v) < n0
    assert sum(1 for c in range(4) for v in world.S(0, 1, 1, 0)[c] if v) > 100 and sum(1 for c in range(4) for v in world.S(0, 6, 1, 0)[c] if v) > 1000
    assert world.K[1].depth != K.depth
    for c in (2, 3):                                                               # sites in the first and last bin of 25 and next to the tile cuts
        assert S0[c][0] and any(S0[c][-8:])
    assert any(S0[3][world.T - 3:world.T + 3]) and any(S0[3][2 * world.T - 3:2 * world.T + 3])


# ---- 1. bins against the model ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mask,md,cpg", GRID, ids=GRID_IDS)
def test_bins_against_the_model(world, mode, mask, md, cpg):
    h, S = world.handle(mode, mask, cpg), world.S(mode, mask, md, cpg)
    for B in (1, 2, 25, 63, 64, 65, 1000, 1024, 4096, 2 * world.T + 67, 1 << 31):
        for c in range(4):
            assert got_bins(h, c, B, md) == R.bin_sums(S, c, B), (B, c)
        assert got_wig(h, world.dir / "t.wig", B, md) == R.wig_text(world.names, S, B).encode(), B


# ---- 2. regions against the model -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,mask,md,cpg", GRID, ids=GRID_IDS)
def test_regions_against_the_model(world, mode, mask, md, cpg):
    h, S = world.handle(mode, mask, cpg), world.S(mode, mask, md, cpg)
    ivs = intervals(world)
    memo = {}
    def want_of(c, a, b):
        if (c, a, b) not in memo:
            memo[(c, a, b)] = R.interval_sums(S, c, a, b)
        return memo[(c, a, b)]
    got = got_regions(h, [iv[:3] for iv in ivs], md)                                    # one call, the order kept
    assert got == [want_of(*iv[:3]) for iv in ivs]
    assert sum(1 for s in got if s[0]) > 60 and sum(1 for s in got if not s[0]) >= 6
    bed = str(world.dir / "r.bed")
    open(bed, "w").write(bed_text(world, ivs))
    recs, dropped = R.parse_bed(bed_text(world, ivs), world.names, world.lens)
    text, nw, nd = got_region_file(h, bed, world.dir / "r.txt", md)
    assert (nw, nd) == (len(ivs), 0) == (len(recs), dropped)
    assert text == R.region_text(world.names, S, recs).encode()


# ---- 3. ties to existing, pinned code ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cpg", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_ties_to_the_report(world, mode, cpg):
    for mask in MASKS:
        h = world.handle(mode, mask, cpg)
        for md in DEPTHS:
            whole = got_regions(h, [(c, 0, world.lens[c]) for c in range(4)], md)
            for c in range(4):
                rows, cov, sd = got_report(h, c, md, 1)
                assert (whole[c][0], whole[c][2]) == (cov, sd), (mask, md, c)
                b1 = got_bins(h, c, 1, md)
                assert [(j, s[1], s[2]) for j, s in enumerate(b1) if s[0]] == rows and all(s[0] <= 1 for s in b1)
                for B in (25, 1000):
                    nb = world.lens[c] // B + 1
                    assert got_bins(h, c, B, md) == got_regions(h, [(c, j * B, min((j + 1) * B, world.lens[c])) for j in range(nb)], md), (B, c)
            assert sum(s[0] for s in whole) > 50


GOLD = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio.json.gz"), "rt"))


@pytest.mark.parametrize("opts", [["-z"], ["-z", "-g", "-r", "-u", "-m", "2"]], ids=["z", "z_g_r_u_m2"])
def test_tie_to_the_pinned_tables(opts, tmp_path, capsys):
    """mode off, on real bsmap output: the B = 1 wiggle lines are the positions and ratios of the pinned -z table of the v2.6 script, and
    whole-chromosome regions hold the `covered cytosines` of its summary line"""
    from bsmap_amd import methratio
    case = GOLD["cases"]["se"]
    run = [r for r in case["runs"] if r["options"] == opts][0]
    fa, bsp, bed = str(tmp_path / "g.fa"), str(tmp_path / "se.bsp"), str(tmp_path / "whole.bed")
    open(fa, "w").write(GOLD["fasta"])
    open(bsp, "w").write(case["files"]["se.bsp"])
    open(bed, "w").write("chr2\t0\t4000000000\nchr1\t0\t4000000000\tfirst\n")
    out, wig, reg = (str(tmp_path / n) for n in ("t.txt", "t.wig", "r.txt"))
    methratio.main(["-q", "-o", out, "-d", fa] + opts + ["-w", wig, "-b", "1", "--regions", bed, "--region-out", reg, bsp])
    assert capsys.readouterr().out == run["stdout"] and open(out).read() == run["table"]
    pinned = [l.split("\t") for l in run["table"].split("\n")[1:-1]]
    want = ["track type=wiggle_0"]
    for name in sorted({f[0] for f in pinned}):
        want.append("variableStep chrom=%s span=1" % name)
        want += ["%s\t%s" % (f[1], f[4]) for f in pinned if f[0] == name]
    assert open(wig).read().split("\n")[:-1] == want and len(want) > 20000
    rows = [l.split("\t") for l in open(reg).read().split("\n")[1:-1]]
    lens = {n: str(len(s)) for n, s in methratio.load_reference(fa, None).items()}
    assert [r[:4] for r in rows] == [["chr2", "0", lens["chr2"], "."], ["chr1", "0", lens["chr1"], "first"]]   # clipped to the chromosomes
    covered = int(run["stdout"].split(" covered cytosines")[0].split()[-1])
    assert sum(int(r[4]) for r in rows) == covered == len(pinned)
    assert sum(int(r[5]) for r in rows) == sum(int(f[6]) for f in pinned) and sum(int(r[6]) for r in rows) == sum(int(f[5]) for f in pinned)


# ---- 4. contention and determinism --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_contention_and_determinism(world, mode):
    """4 096 copies of the whole long chromosome in one call: every tile of every copy adds to its copy's cells, and integer sums come out the same
    bits whatever the order"""
    h, S = world.handle(mode, 0, 0), world.S(mode, 0, 1, 0)
    n = world.lens[3]
    want = R.interval_sums(S, 3, 0, n)
    assert want[0] > 1000
    ivs = [(3, 0, n)] * 4096
    first = got_regions(h, ivs, 1)
    assert first == [want] * 4096
    assert got_regions(h, ivs, 1) == first
    a, b = got_wig(h, world.dir / "d1.wig", 25, 1), got_wig(h, world.dir / "d2.wig", 25, 1)
    assert a == b and len(a) > 1000


@pytest.mark.parametrize("mode", [0, 1])
def test_intervals_of_many_tiles(tmp_path, mode):
    """a launch that is mostly intervals of 64 tiles and more takes the kernel's wide blocks (16 tiles meet in LDS ahead of the adds): one chromosome of
    65 T + 13 letters, three copies of the whole of it, one that starts and ends inside a tile, and a short one beside them"""
    T = _lib().bsx_meth_region_tile()
    rng = np.random.default_rng(5)
    n = 65 * T + 13
    ref = "".join(rng.choice(list("ACGT"), n).tolist())
    snp = {i: 0.5 for i in rng.integers(0, n, 400).tolist() if ref[i] in "CG"}
    alns = []
    for k in range(3000):
        pos, L, st = int(rng.integers(0, n - 60)), int(rng.integers(30, 61)), k % 4
        alns.append((0, pos, st, 0, -1, make_read(rng, ref, snp, pos, L, st)))
    K = M.pileup([ref], alns, 2)
    S = R.site_table(K, 1, mode, 0)
    fa = str(tmp_path / "long.fa")
    open(fa, "w").write(">long\n" + ref + "\n")
    ivs = [(0, 0, n), (0, T // 2, n - T // 2), (0, 0, n), (0, 100, 160), (0, 0, n)]
    h = handle(fa, snp=bool(mode))
    try:
        h.add(alns, 2)
        rule(h, mode, 0)
        want = [R.interval_sums(S, *iv) for iv in ivs]
        got = got_regions(h, ivs, 1)
        assert got == want and want[0][0] > 10000 and want[1] != want[0]
        assert got_regions(h, ivs, 1) == got
        rows, cov, sd = got_report(h, 0, 1, 1)
        assert (got[0][0], got[0][2]) == (cov, sd) and got[0][1] == sum(r[1] for r in rows)
    finally:
        h.close()


# ---- 5. borders between chromosomes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_borders_between_chromosomes(tmp_path, mode):
    """...C | G...: in the concatenated arrays the two letters read CG.  No bin or interval of the first chromosome holds a count of the second, and the
    last C of the first is in no CG context"""
    refs, names = ["TTACGTTAC", "GTTACGTT"], ["x1", "x2"]
    fa = str(tmp_path / "two.fa")
    open(fa, "w").write(">x1\nTTACGTTAC\n>x2\nGTTACGTT\n")
    alns = [(0, 0, 0, 0, -1, "TTACGTTAC"), (0, 0, 0, 0, -1, "TTATGTTAC"), (0, 0, 1, 0, -1, "TTACGTTAC"), (0, 1, 3, 0, -1, "TACGTTAT"),
            (1, 0, 1, 0, -1, "GTTACGTT"), (1, 0, 1, 0, -1, "GTTACATT"), (1, 0, 1, 0, -1, "ATT"), (1, 0, 0, 0, -1, "GTTACGTT"), (1, 0, 2, 0, -1, "GTTAC")]
    K = M.pileup(refs, alns, 0)
    assert K.depth[0][8] == 2 and K.depth[1][0] == 3 and K.meth[1][0] == 2
    h = handle(fa, snp=bool(mode))
    try:
        h.add(alns, 0)
        for mask in (0, 1, 6, 8):
            rule(h, mode, mask)
            S = R.site_table(K, 1, mode, mask)
            for B in (1, 4, 9, 8, 16, 64):
                for c in range(2):
                    assert got_bins(h, c, B, 1) == R.bin_sums(S, c, B), (mask, B, c)
            ivs = [(0, 0, 9), (0, 8, 9), (0, 5, 200), (1, 0, 8), (1, 0, 1), (0, 9, 9), (1, 0, 0)]
            assert got_regions(h, ivs, 1) == [R.interval_sums(S, *iv) for iv in ivs], mask
        S_cg, S_other = R.site_table(K, 1, mode, 1), R.site_table(K, 1, mode, 8)
        assert S_cg[0][8] is None and S_other[0][8] and S_cg[0][3] and S_cg[1][0] is None and S_other[1][0]   # the border letters are in class 3
        rule(h, mode, 0)
        assert got_regions(h, [(0, 8, 9)], 1)[0][:3] == [1, 2, 2] and got_regions(h, [(1, 0, 1)], 1)[0][:3] == [1, 2, 3]
    finally:
        h.close()


# ---- 6. state --------------------------------------------------------------------------------------------------------------------------------
def test_the_calls_change_nothing(world):
    h = world.handle(1, 0, 1)
    before = got_table(h, world.dir / "before.txt")
    got_bins(h, 3, 25, 1); got_regions(h, [(3, 0, world.lens[3]), (2, 5, 50)], 1)
    got_wig(h, world.dir / "s.wig", 64, 3)
    open(world.dir / "s.bed", "w").write("wa_long\t0\t100\n")
    got_region_file(h, world.dir / "s.bed", world.dir / "s.txt", 1)
    assert got_table(h, world.dir / "after.txt") == before and before[1] > 1000
    assert before[0].decode() == M.table(world.names, world.K[1], 1, True, 1)[0]


def test_argument_errors(world):
    h = world.handle(0, 0, 0)
    L, hh = h.L, h.h
    one = np.zeros(8, np.uint32)
    out = np.zeros(40, np.uint64)
    n = C.c_uint64()
    ptr = lambda a: a.ctypes.data
    def regions(c, a, b, n_=1, sums=out):
        ca, sa, ea = np.array([c], np.uint32), np.array([a], np.uint32), np.array([b], np.uint32)
        return L.bsx_meth_regions(hh, n_, ptr(ca), ptr(sa), ptr(ea), 1, ptr(sums) if sums is not None else None)
    assert regions(4, 0, 1) == BSX_ERR_ARG and regions(0xFFFFFFFF, 0, 1) == BSX_ERR_ARG          # chr out of range
    assert regions(3, 5, 4) == BSX_ERR_ARG                                                        # start > end
    assert regions(3, 0, 5, sums=None) == BSX_ERR_ARG and L.bsx_meth_regions(None, 1, ptr(one), ptr(one), ptr(one), 1, ptr(out)) == BSX_ERR_ARG
    assert L.bsx_meth_regions(hh, 1, None, ptr(one), ptr(one), 1, ptr(out)) == BSX_ERR_ARG
    assert L.bsx_meth_regions(hh, 0, None, None, None, 1, None) == 0                              # n == 0
    assert regions(3, 0, 0xFFFFFFFF) == 0 and out[:5].tolist() == R.interval_sums(world.S(0, 0, 1, 0), 3, 0, world.lens[3])   # end is clipped
    assert L.bsx_meth_bins(hh, 4, 25, 1, 40, ptr(out), C.byref(n)) == BSX_ERR_ARG and L.bsx_meth_bins(hh, 3, 0, 1, 40, ptr(out), C.byref(n)) == BSX_ERR_ARG
    assert L.bsx_meth_bins(hh, 1, 1, 1, 5, ptr(out), C.byref(n)) == BSX_ERR_ARG and n.value == 6  # the cap is too small: the size comes back
    assert L.bsx_meth_bins(hh, 1, 1, 1, 6, ptr(out), None) == BSX_ERR_ARG and L.bsx_meth_bins(None, 1, 1, 1, 6, ptr(out), C.byref(n)) == BSX_ERR_ARG
    assert L.bsx_meth_bins(hh, 1, 1, 1, 8, ptr(out), C.byref(n)) == 0 and n.value == 6
    assert L.bsx_meth_write_wig(hh, str(world.dir / "e.wig").encode(), 0, 1) == BSX_ERR_ARG and not os.path.exists(world.dir / "e.wig")
    assert L.bsx_meth_write_wig(hh, None, 25, 1) == BSX_ERR_ARG and L.bsx_meth_write_regions(hh, None, b"x", 1, None, None) == BSX_ERR_ARG
    assert L.bsx_meth_write_regions(hh, str(world.dir / "absent.bed").encode(), str(world.dir / "e.txt").encode(), 1, None, None) == BSX_ERR_IO
    assert not os.path.exists(world.dir / "e.txt")


def test_before_any_alignment(world, tmp_path):
    h = handle(world.fa)
    try:
        assert got_regions(h, [(3, 0, world.lens[3]), (0, 0, 1)], 1) == [[0] * 5] * 2
        assert got_bins(h, 2, 25, 1) == [[0] * 5] * (4099 // 25 + 1)
        assert got_wig(h, tmp_path / "z.wig", 25, 1).decode() == "track type=wiggle_0\n" + "".join("variableStep chrom=%s span=25\n" % n for n in sorted(world.names))
        open(tmp_path / "z.bed", "w").write("wb_mid\t0\t10\tz\n")
        assert got_region_file(h, tmp_path / "z.bed", tmp_path / "z.txt", 1) == ((R.REGION_HEADER + "wb_mid\t0\t10\tz\t0\t0\t0\t0.00\tNA\tNA\tNA\n").encode(), 1, 0)
    finally:
        h.close()


# ---- 7. command line -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bsp", "sam"])
def test_command_line(fmt, tmp_path, capsys):
    """the §3.8 edge set as a SAM and as a BSP file through methratio.main: the table, the wiggle file and the region file equal the model's"""
    import test_gpu_methratio_ctsnp as CT
    from bsmap_amd import methratio
    e = CT.Edges()
    fa, path = str(tmp_path / "edges.fa"), str(tmp_path / ("in." + fmt))
    open(fa, "w").write(e.fasta)
    with open(path, "w") as f:
        if fmt == "sam":
            f.write("".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(r)) for n, r in zip(e.names, e.refs)))
        for k, (c, pos, st, insert, cut, s) in enumerate(e.alns):
            if fmt == "sam":
                f.write("r%d\t0\t%s\t%d\t255\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:0\tZS:Z:%s\n" % (k, e.names[c], pos + 1, len(s), cut + 1, insert, s, "I" * len(s), STRANDS[st]))
            else:
                f.write("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t%d\n" % (k, s, "I" * len(s), e.names[c], pos + 1, STRANDS[st], insert))
    bed_text_ = "# targets\nedgeC\t0\t2100\twhole\nedgeA 290 400 tail\nabsent\t0\t5\nedgeB\t0\t97\nedgeC\t1000\t1100\nedgeC\t1500\t1560\tsnps\r\nedgeA\t0\t0"
    bed = str(tmp_path / "t.bed")
    open(bed, "w", newline="").write(bed_text_)
    out, wig, reg = (str(tmp_path / n) for n in ("t.txt", "t.wig", "r.txt"))
    alns = e.alns if fmt == "sam" else [(c, pos, st, insert, -1, s) for c, pos, st, insert, cut, s in e.alns]
    for extra, mode, mask, cpg, md in ((["-i", "correct", "-x", "CG,CHG"], 1, 3, 0, 1), (["-g", "-m", "2"], 0, 0, 1, 2)):
        methratio.main(["-q", "-z", "-r", "-o", out, "-d", fa] + extra + ["-w", wig, "-b", "50", "--regions", bed, "--region-out", reg, path])
        stdout = capsys.readouterr().out
        K = M.pileup(e.refs, alns, 2, True)
        if cpg:
            K = M.combine_cpg(K)
        table, nc, nd = M.table(e.names, K, md, True, mode, mask)
        S = R.site_table(K, md, mode, mask)
        recs, dropped = R.parse_bed(bed_text_, e.names, [len(r) for r in e.refs])
        assert open(out).read() == table and stdout == M.summary(K.nmap, nc, nd) and dropped == 1 and len(recs) == 6
        assert open(wig).read() == R.wig_text(e.names, S, 50) and open(reg).read() == R.region_text(e.names, S, recs)
        # without the options: the table and the summary of the parent's option set
        methratio.main(["-q", "-z", "-r", "-o", out, "-d", fa] + extra + [path])
        assert (capsys.readouterr().out, open(out).read()) == (stdout, table)
    # a bad line: the error names it and no region file is written
    from bsmap_amd import BsxError
    open(bed, "w").write("edgeA\t0\t5\n\nedgeA\t9\t5\n")
    os.remove(reg)
    with pytest.raises(BsxError) as x:
        methratio.main(["-q", "-o", out, "-d", fa, "--regions", bed, "--region-out", reg, path])
    assert x.value.code == BSX_ERR_IO and "line 3" in str(x.value) and not os.path.exists(reg)
