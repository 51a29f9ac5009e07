"""The two-sample interval sums where a whole-genome run takes them (bsx_meth_diff_regions / bsx_meth_regions through meth_tiled, bsx_meth_write_diff_bins, the sums
of bsx_meth_diff_dmrs): the blocks of sixteen waves, context masks and -g, a call that is cut into launches at 2^22 intervals or tiles, and a
bin file of more than 2^22 bins.

Integers come from pinned code: the rows are the join of a.report() and b.report() (meth_util.joined), the sums are Python or numpy integer sums of them.  p is
compared with the exact model of diff_model.py where an interval's support is at most 2 501 tables (the size test_gpu_methdiff.py holds); everywhere p is NaN exactly
where N == 0, inside [0, 1] otherwise, and has the same bits for the same sums.  The seeds are such that the model leaves out no case as near the selection limit."""
import math

import numpy as np
import pytest

import diff_model as D
import meth_util as U
from bsmap_amd.methratio import Meth, _bind

pytestmark = pytest.mark.gpu
CHUNK = 1 << 22          # REGION_CHUNK of bsx_meth.hip: a launch holds fewer than this many intervals and tiles before its last interval
LONG_TILES = 64          # the wide rule: 2 (tiles of intervals of 64 tiles and more) > tiles
MAX_SUPPORT = 2501
LETTERS = np.frombuffer(b"ACGT", np.uint8)


# ---- the model's side ------------------------------------------------------------------------------------------------------------------------------
def n_tiles(length, T):
    return (np.asarray(length, np.int64) + T - 1) // T


def clipped_lengths(lens, chr, start, end):
    chr, start, end = (np.asarray(x, np.int64) for x in (chr, start, end))
    e = np.minimum(end, np.asarray(lens, np.int64)[chr])
    return e - np.minimum(start, e)


def launch_cuts(nt, chunk=CHUNK):
    """the launches of a call restated from the tile counts of its intervals: a launch takes intervals while it holds fewer than `chunk` of them and of tiles"""
    cum = np.concatenate([[0], np.cumsum(nt)])
    cuts = [0]
    while cuts[-1] < len(nt):
        a = cuts[-1]
        cuts.append(int(min(np.searchsorted(cum, cum[a] + chunk, "left"), a + chunk, len(nt))))
    return cuts


def is_wide(nt):
    nt = np.asarray(nt, np.int64)
    return 2 * int(nt[nt >= LONG_TILES].sum()) > int(nt.sum())


def model_sums(rows_by_chr, lens, chr, start, end):
    """int64 [n][5]: U.interval_sums by prefix sums over the rows (for calls of thousands of intervals)"""
    chr, start, end = (np.asarray(x, np.int64) for x in (chr, start, end))
    out = np.zeros((len(chr), 5), np.int64)
    for c, rows in enumerate(rows_by_chr):
        pick = np.nonzero(chr == c)[0]
        if not len(pick) or not rows:
            continue
        pos = np.array([r[0] for r in rows], np.int64)
        cum = np.vstack([np.zeros((1, 5), np.int64), np.cumsum(np.array([(1,) + tuple(r[1:]) for r in rows], np.int64), 0)])
        e = np.minimum(end[pick], lens[c])
        s = np.minimum(start[pick], e)
        out[pick] = cum[np.searchsorted(pos, e)] - cum[np.searchsorted(pos, s)]
    return out


def single_sample_sums(m, lens, ivs, min_depth=1):
    """[[N, M, D, E, MC]] of bsx_meth_regions without the C/T-SNP mode (E = D << 16, MC = M << 16) from the pinned report"""
    rows = []
    for c in range(len(lens)):
        pos, dep, met, _, _ = m.report(c, min_depth, True)
        rows.append([(int(x), int(k), int(d), int(d) << 16, int(k) << 16) for x, d, k in zip(pos, dep, met)])
    return U.interval_sums(rows, lens, ivs)


def small_support(s):
    """s: [N, MA, DA, MB, DB] of the model.  True where the interval has a site and its support is of the size that the exact model holds"""
    lo, hi = D.support(*s[1:])
    return bool(s[0]) and hi - lo + 1 <= MAX_SUPPORT


def distinct_small(sums):
    """how many distinct (MA, DA, MB, DB) of the model's `sums` check_p holds to the exact model"""
    return len({tuple(s[1:]) for s in np.asarray(sums).tolist() if small_support(s)})


def check_p(sums, p):
    """sums: [n][5] of the model; p: the library's.  Returns how many distinct (MA, DA, MB, DB) were held to the exact model: every one whose support is at most
    2 501 tables"""
    bits = {}
    exact = 0
    for s, x, b in zip(np.asarray(sums).tolist(), p.tolist(), p.view(np.uint64).tolist()):
        if not s[0]:
            assert math.isnan(x), (s, x)
            continue
        assert 0.0 <= x <= 1.0, (s, x)
        assert bits.setdefault(tuple(s[1:]), b) == b, s      # equal sums, equal bits
    for quad, b in bits.items():
        lo, hi = D.support(*quad)
        if hi - lo + 1 <= MAX_SUPPORT:
            assert not D.near_boundary(*quad), quad           # the seeds' promise: the model leaves out none
            err = D.p_error(float(np.array([b], np.uint64).view(np.float64)[0]), quad)
            assert err is None, err
            exact += 1
    return exact


def make_read(rng, ref, c, pos, n, st, level):
    match, convert = ("C", "T") if st % 2 == 0 else ("G", "A")
    return (c, pos, st, 0, -1, "".join(convert if x == match and rng.random() >= level else x for x in ref[pos:pos + n]))


def make_pair(fa, alns, mask=0, cpg=False):
    a, b = Meth.from_fasta(fa), Meth.from_fasta(fa)
    for m, reads in zip((a, b), alns):
        m.set_contexts(mask)
        m.add(reads, 0)
        if cpg:
            m.combine_cpg()
    return a, b


def arrays(ivs):
    return [np.array([v[k] for v in ivs], np.uint32) for k in range(3)]


# ---- world "wide" ------------------------------------------------------------------------------------------------------------------------------------
class Wide:
    """Two sequences, the sorted names not in id order: 65 T + 13 letters (T = bsx_meth_region_tile()) and 70.  Random ACGT with CG planted across T - 1 | T and
    16 T - 1 | 16 T (a tile border, and a border of the 16-tile blocks for an interval that starts at 0), a C as the last letter of the long sequence and a G as the first
    of the next.  3 000 reads of 30-60 nt per sample on all four strands at the levels 0.7 and 0.35, reads over every planted site and both ends; [30 T, 33 T) is
    covered in A only.  `flat`: the same positions with A's reads fully methylated and B's fully converted."""
    NAMES = ["wz_long", "wa_next"]
    LONG, NEXT = 0, 1

    def __init__(self, tmp, T):
        rng = np.random.default_rng(67)
        self.T, self.n = T, 65 * T + 13
        long, nxt = LETTERS[rng.integers(0, 4, self.n)].copy(), LETTERS[rng.integers(0, 4, 70)].copy()
        for at in (T - 1, 16 * T - 1):
            long[at], long[at + 1] = ord("C"), ord("G")
        long[-1], nxt[0] = ord("C"), ord("G")
        self.refs = [long.tobytes().decode(), nxt.tobytes().decode()]
        self.lens = [self.n, 70]
        self.planted = (T - 1, 16 * T - 1)
        self.a_only = (30 * T, 33 * T)
        self.fa = U.write_fasta(tmp / "wide.fa", self.NAMES, self.refs)
        self.alns = [self.reads(rng, 0.7, True), self.reads(rng, 0.35, False)]
        rng = np.random.default_rng(68)
        self.flat = [self.reads(rng, 1.0, True), self.reads(rng, 0.0, False)]

    def reads(self, rng, level, is_a):
        out, n = [], self.n
        for _ in range(3000):
            k = int(rng.integers(30, 61))
            pos, st = int(rng.integers(0, n - k + 1)), int(rng.integers(0, 4))
            if is_a or pos + k <= self.a_only[0] or pos >= self.a_only[1]:
                out.append(make_read(rng, self.refs[0], 0, pos, k, st, level))
        for st in (0, 1, 0, 1, 3, 2):      # every planted site and every end three deep on both reference strands
            out += [make_read(rng, self.refs[0], 0, at - 19, 40, st, level) for at in self.planted + (19, 139, n - 21)]
            out += [make_read(rng, self.refs[1], 1, at, 40, st, level) for at in (0, 30)]
        return out

    def intervals(self):
        """the wide list of the issue: three copies of the whole long sequence, one that starts and ends inside a tile, a short one and the other sequence"""
        T, n = self.T, self.n
        return [(0, 0, n), (0, T // 2, n - T // 2), (0, 0, n), (0, 100, 160), (1, 0, 70), (0, 0, n)]

    def border_intervals(self):
        """short ones that end between the C and the G of each planted CG, the last position of the long sequence and the first of the next"""
        T, n = self.T, self.n
        return [(0, T - 40, T), (0, T, T + 40), (0, 16 * T - 1, 16 * T), (0, n - 1, n), (1, 0, 1)]


@pytest.fixture(scope="module")
def wide(tmp_path_factory):
    return Wide(tmp_path_factory.mktemp("wide"), _bind().bsx_meth_region_tile())


@pytest.fixture(scope="module")
def wide_both(wide):
    a, b = make_pair(wide.fa, wide.alns)
    rows = {md: [U.joined(a, b, c, md) for c in range(2)] for md in (1, 3)}
    yield a, b, rows
    a.close()
    b.close()


def test_the_wide_world_is_what_it_says(wide, wide_both):
    """from the model alone: what the tests below rely on"""
    a, b, rows = wide_both
    T, n = wide.T, wide.n
    assert T == 2048 and a.write_order() == [1, 0]
    pos = [{r[0] for r in rows[1][c]} for c in range(2)]
    assert {T - 1, T, 16 * T - 1, 16 * T, n - 1} <= pos[0] and 0 in pos[1]
    assert len(pos[0]) > 5000 and 0 < len(rows[3][0]) < len(pos[0]) // 4 and len(pos[1]) > 10
    lo, hi = wide.a_only
    assert not any(lo <= x < hi for x in pos[0]) and sum(lo <= int(x) < hi for x in a.report(0)[0]) > 500    # covered in A only
    assert all(min(x for x in pos[0] if x >= k * T) < (k + 1) * T for k in range(65) if not 29 <= k <= 33)     # common sites in the tiles all along


def test_wide_blocks(wide, wide_both):
    a, b, rows = wide_both
    ivs = wide.intervals()
    nt = n_tiles(clipped_lengths(wide.lens, *arrays(ivs)), wide.T)
    assert nt.tolist() == [66, 65, 66, 1, 1, 66] and launch_cuts(nt) == [0, 6] and is_wide(nt)      # one launch, and it takes the blocks of sixteen waves
    assert (int(nt[0]) - 1) // 16 == int(nt[0]) // 16                       # the first interval's last tile and the second's first share a block
    for md in (1, 3):
        want = U.interval_sums(rows[md], wide.lens, ivs)
        assert model_sums(rows[md], wide.lens, *arrays(ivs)).tolist() == want
        sums, p = a.diff_regions(b, *arrays(ivs), md)
        assert sums.dtype == np.uint64 and sums.tolist() == want, md
        assert want[0] == want[2] == want[5] and 0 < want[1][0] < want[0][0] and want[3][0] >= 2 - md // 2 and want[4][0] > 10
        assert check_p(want, p) >= 2
        again = a.diff_regions(b, *arrays(ivs), md)
        assert sums.tobytes() == again[0].tobytes() and p.tobytes() == again[1].tobytes()


def test_narrow_and_wide_agree(wide, wide_both):
    """each long interval among 2 100 intervals of one tile: the launch takes the blocks of four waves, and gives the sums and the bits of p of the wide launch"""
    a, b, rows = wide_both
    T, n = wide.T, wide.n
    ivs = wide.intervals()
    wide_sums, wide_p = a.diff_regions(b, *arrays(ivs))
    rng = np.random.default_rng(3)
    for k, at in ((0, 0), (1, 1000), (5, 2100)):      # every long interval of the list; its entry 2 is entry 0 once more (the same cells, the same place as k = 0)
        start = rng.integers(0, n - T, 2100)
        small = [(0, int(s), int(s) + int(ln)) for s, ln in zip(start, rng.integers(1, T + 1, 2100))]
        mixed = small[:at] + [ivs[k]] + small[at:]
        nt = n_tiles(clipped_lengths(wide.lens, *arrays(mixed)), T)
        assert int(nt.max()) == int(nt[at]) >= LONG_TILES and int(nt.sum()) == 2100 + int(nt[at]) and not is_wide(nt) and launch_cuts(nt) == [0, 2101]
        sums, p = a.diff_regions(b, *arrays(mixed))
        assert sums[at].tolist() == wide_sums[k].tolist() and p[at:at + 1].tobytes() == wide_p[k:k + 1].tobytes()
        want = model_sums(rows[1], wide.lens, *arrays(mixed))
        assert np.array_equal(sums.astype(np.int64), want)
        ones = np.delete(want, at, 0)       # the intervals of one tile: the model says that nearly all hold a site, and every one a support the exact model takes
        assert all(small_support(s) for s in ones.tolist() if s[0]) and distinct_small(ones) > 1500
        assert check_p(want, p) >= distinct_small(ones)


@pytest.mark.parametrize("mask,cpg", [(1, False), (6, False), (8, False), (1, True), (0, True)], ids=["CG", "CHG-CHH", "CN", "CG-g", "all-g"])
def test_masks_and_combined_cpg(wide, wide_both, mask, cpg):
    T, n = wide.T, wide.n
    base = [{r[0]: r[1:] for r in rows} for rows in wide_both[2][1]]
    a, b = make_pair(wide.fa, wide.alns, mask, cpg)
    try:
        ivs = wide.intervals() + wide.border_intervals()
        for md in (1, 3):
            rows = [U.joined(a, b, c, md) for c in range(2)]
            want = U.interval_sums(rows, wide.lens, ivs)
            by = [{r[0]: r[1:] for r in r_c} for r_c in rows]
            if md == 1:      # the model first
                assert 0 < len(by[0]) != len(base[0]) and (cpg or set(by[0]) < set(base[0])) and want[0][0] == len(by[0])
                if mask == 1 and not cpg:     # the C at T - 1 is in a CG although its G lies in the next tile and outside the interval
                    assert by[0][T - 1] == base[0][T - 1] and want[6][0] >= 1 and want[8] == [1] + list(base[0][16 * T - 1])
                    assert n - 1 not in by[0] and 0 not in by[1] and want[9] == want[10] == [0] * 5
                if mask == 8:                 # the last C of a sequence and the first G of the next look at no letter: class CN, whatever follows in memory
                    assert by[0][n - 1] == base[0][n - 1] and by[1][0] == base[1][0] and want[9][0] == want[10][0] == 1
                    assert T - 1 not in by[0] and T not in by[0]
                if cpg:                       # the G's cell is empty and the C carries both
                    for at in wide.planted:
                        assert at + 1 not in by[0] and by[0][at] == tuple(x + y for x, y in zip(base[0][at], base[0][at + 1]))
                    assert want[6][1:] != U.interval_sums(wide_both[2][1], wide.lens, ivs[6:7])[0][1:]      # (T - 40, T) holds the counts of the G behind its end
                    if mask == 0:             # no fold across the sequences' border
                        assert by[0][n - 1] == base[0][n - 1] and by[1][0] == base[1][0]
            sums, p = a.diff_regions(b, *arrays(ivs), md)
            assert sums.tolist() == want, (mask, cpg, md)
            short = [want[i] for i in (3, 4, 6, 7, 8, 9, 10) if want[i][0]]      # the model: every short interval with a site has a support the exact model takes
            assert all(small_support(s) for s in short) and distinct_small(short) >= 2 - md // 2
            assert check_p(want, p) >= distinct_small(short)
    finally:
        a.close()
        b.close()


def test_contention(wide, wide_both):
    """4 096 copies of the whole long sequence in one call: 16 896 blocks of sixteen waves add to 4 096 sets of cells, and integer sums are the same bits in any order"""
    a, b, rows = wide_both
    ivs = [(0, 0, wide.n)] * 4096
    want = U.interval_sums(rows[1], wide.lens, ivs[:1])[0]
    nt = n_tiles(clipped_lengths(wide.lens, *arrays(ivs)), wide.T)
    assert is_wide(nt) and launch_cuts(nt) == [0, 4096] and want[0] > 5000
    sums, p = a.diff_regions(b, *arrays(ivs))
    assert np.array_equal(sums.astype(np.int64), np.array([want] * 4096, np.int64))
    assert check_p([want] * 4096, p) == distinct_small([want])      # 0 if the whole sequence's support is beyond the exact model: then p is held as one value in [0, 1]
    one = a.diff_regions(b, *arrays(ivs[:1]))                        # ... with the bits that a call of this one interval gives
    assert one[0].tolist() == [want] and p.view(np.uint64).tolist() == one[1].view(np.uint64).tolist() * 4096
    again = a.diff_regions(b, *arrays(ivs))
    assert sums.tobytes() == again[0].tobytes() and p.tobytes() == again[1].tobytes()


def test_dmr_sums_take_the_wide_path(wide):
    """A fully methylated, B fully converted: with max_q 1 and any gap every sequence is one run from its first to its last common site; the long one spans
    64 tiles and more, so the DMRs' sums come from the blocks of sixteen waves"""
    a, b = make_pair(wide.fa, wide.flat)
    try:
        rows = [U.joined(a, b, c, 1) for c in range(2)]
        assert all(r[1] == r[2] and r[3] == 0 for r_c in rows for r in r_c) and len(rows[0]) > 5000 and len(rows[1]) > 10
        want_runs = [(c, rows[c][0][0], rows[c][-1][0] + 1, len(rows[c])) for c in a.write_order()]
        nt = n_tiles([r[2] - r[1] for r in want_runs], wide.T)
        assert int(nt.max()) >= LONG_TILES and is_wide(nt)
        store = a.diff_report_all(b)
        assert len(store[1]) == len(rows[0]) + len(rows[1])
        chr, start, end, n_sig, sums, p = a.diff_dmrs(b, 1.0, 0, 0xFFFFFFFF, 1)
        assert list(zip(chr.tolist(), start.tolist(), end.tolist(), n_sig.tolist())) == want_runs
        want = U.interval_sums(rows, wide.lens, [r[:3] for r in want_runs])
        assert sums.tolist() == want and [w[0] for w in want] == [r[3] for r in want_runs]
        ref_sums, ref_p = a.diff_regions(b, chr, start, end)
        assert sums.tobytes() == ref_sums.tobytes() and p.tobytes() == ref_p.tobytes()
        assert small_support(want[0]) and check_p(want, p) >= 1      # the run of the sequence of 70 letters (first in the sorted names) is held to the exact model
    finally:
        a.close()
        b.close()


# ---- world "cuts" ------------------------------------------------------------------------------------------------------------------------------------
class Cuts:
    """One sequence of 2^22 + 77 letters and one of 50: the letter A but for clusters of random ACGT (a few hundred C and G), each under reads of 40 nt on all four
    strands in both samples: at position 0, across T, across 5 T (300 letters), across 2^22 (with CG at 2^22 - 1 | 2^22) and over the last 40 letters (the last one a
    C); one more cluster, at 3 T + 100, is covered in A only."""
    NAMES = ["cz_long", "ca_short"]

    def __init__(self, tmp, T):
        rng = np.random.default_rng(71)
        self.T, self.n = T, CHUNK + 77
        n = self.n
        self.clusters = [(0, 60), (T - 40, 80), (5 * T - 100, 300), (CHUNK - 30, 60), (n - 40, 40)]
        self.a_only = (3 * T + 100, 60)
        long = np.full(n, ord("A"), np.uint8)
        for s, k in self.clusters + [self.a_only]:
            long[s:s + k] = LETTERS[rng.integers(0, 4, k)]
        long[0] = long[CHUNK - 1] = long[n - 1] = long[T - 1] = ord("C")
        long[CHUNK] = long[T] = ord("G")
        assert 200 < int(np.isin(long, LETTERS[1:3]).sum()) < 600
        self.refs = [long.tobytes().decode(), LETTERS[rng.integers(0, 4, 50)].tobytes().decode()]
        self.lens = [n, 50]
        self.fa = U.write_fasta(tmp / "cuts.fa", self.NAMES, self.refs)
        self.alns = [self.reads(rng, 0.7, True), self.reads(rng, 0.35, False)]

    def reads(self, rng, level, is_a):
        out = []
        for s, k in self.clusters + ([self.a_only] if is_a else []):
            for pos in sorted(set(list(range(s, s + k - 39, 7)) + [s + k - 40])):
                out += [make_read(rng, self.refs[0], 0, pos, 40, st, level) for st in (0, 1, 2, 3)]
        out += [make_read(rng, self.refs[1], 1, pos, 40, st, level) for pos in (0, 10) for st in (0, 1, 2, 3)]
        return out

    def seven(self):
        """two of one tile with sites, one of two tiles, one of three tiles across the cluster at 2^22, an empty one, one without a common site, one clipped"""
        T, n = self.T, self.n
        return [(0, 0, 50), (0, T - 40, T + 40), (0, 0, T + 40), (0, CHUNK - 2 * T, CHUNK + 20), (0, 500, 500), (0, 3 * T + 100, 3 * T + 160), (0, n - 40, n + 1000)]

    def lean(self):
        """the same with the interval of three tiles replaced by one that lies behind the sequence's end: six tiles per seven intervals"""
        ivs = self.seven()
        ivs[3] = (0, self.n + 5, self.n + 9)
        return ivs


@pytest.fixture(scope="module")
def cuts(tmp_path_factory):
    w = Cuts(tmp_path_factory.mktemp("cuts"), _bind().bsx_meth_region_tile())
    a, b = make_pair(w.fa, w.alns)
    w.rows = [U.joined(a, b, c, 1) for c in range(2)]
    yield w, a, b
    a.close()
    b.close()


def test_the_cuts_world_is_what_it_says(cuts):
    w, a, b = cuts
    pos = {r[0] for r in w.rows[0]}
    assert {0, w.T - 1, w.T, CHUNK - 1, CHUNK, w.n - 1} <= pos and 100 < len(pos) < 600 and len(w.rows[1]) > 5
    s, k = w.a_only
    assert not any(s <= x < s + k for x in pos) and sum(s <= int(x) < s + k for x in a.report(0)[0]) > 5
    assert n_tiles(clipped_lengths(w.lens, *arrays(w.seven())), w.T).tolist() == [1, 1, 2, 3, 0, 1, 1]
    assert n_tiles(clipped_lengths(w.lens, *arrays(w.lean())), w.T).tolist() == [1, 1, 2, 0, 0, 1, 1]


def cycled(w, kinds, n, tail=()):
    """interval i is kinds[i % 7] for i < n, then `tail`: (the arrays of the call, i % 7 or 7 + the place in the tail, the tile counts)"""
    table = np.array(list(kinds) + list(tail), np.uint32)
    which = np.concatenate([np.arange(n) % 7, 7 + np.arange(len(tail))]).astype(np.int64)
    iv = [np.ascontiguousarray(table[which, k]) for k in range(3)]
    return iv, which, n_tiles(clipped_lengths(w.lens, *arrays(table.tolist())), w.T)[which]


def run_cycled(w, a, b, sample, kinds, n, tail=()):
    """one call of n + len(tail) intervals against the model of the seven (and the tail's) intervals; returns (sums, p or None)"""
    table = list(kinds) + list(tail)
    iv, which, _ = cycled(w, kinds, n, tail)
    if sample == "pair":
        want = np.array(U.interval_sums(w.rows, w.lens, table), np.uint64)
        small_sums, small_p = a.diff_regions(b, *arrays(table))         # a launch of its own, narrow: p of every kind, held to the exact model
        assert small_sums.tolist() == want.tolist() and check_p(want, small_p) == len({tuple(s[1:]) for s in want.tolist() if s[0]})
        assert len({x for s, x in zip(want.tolist(), small_p.view(np.uint64).tolist()) if s[0]}) >= 4
        sums, p = a.diff_regions(b, *iv)
        assert np.array_equal(sums, want[which])
        assert np.array_equal(p.view(np.uint64), small_p.view(np.uint64)[which])
        assert np.array_equal(np.isnan(p), want[which, 0] == 0)
    else:
        want = np.array(single_sample_sums(a, w.lens, table), np.uint64)
        sums, p = a.regions(*iv), None
    assert np.array_equal(sums, want[which])
    assert sorted({tuple(s) for s in want.tolist()}, reverse=True)[3][0] > 0 and [0] * 5 in want.tolist()    # four distinct sums with sites, and an empty one
    return sums, p


@pytest.mark.parametrize("sample", ["pair", "single"])
def test_cut_with_the_cycle_of_seven(cuts, sample):
    """2^22 + 5 intervals, interval i the i % 7-th of seven: they hold nine tiles per seven intervals, so the first launch is full of tiles after 3 262 235 intervals and
    the second starts in the middle of the cycle, with the empty interval in its first cell"""
    w, a, b = cuts
    n = CHUNK + 5
    _, which, nt = cycled(w, w.seven(), n)
    cut = launch_cuts(nt)
    assert cut == [0, 3262235, n] and which[cut[1]] == 4 and int(nt[:cut[1]].sum()) == CHUNK and not is_wide(nt[:cut[1]])
    run_cycled(w, a, b, sample, w.seven(), n)


@pytest.mark.parametrize("sample", ["pair", "single"])
def test_cut_by_interval_count(cuts, sample):
    """2^22 + 5 intervals of six tiles per seven: the first launch ends at 2^22 intervals, and 2^22 mod 7 = 2, so the second launch (and the second piece of the p
    loop) starts with the interval of two tiles and holds two empty ones"""
    w, a, b = cuts
    n = CHUNK + 5
    _, which, nt = cycled(w, w.lean(), n)
    cut = launch_cuts(nt)
    assert cut == [0, CHUNK, n] and int(nt[:CHUNK].sum()) < CHUNK and which[CHUNK:].tolist() == [2, 3, 4, 5, 6] and nt[CHUNK:].tolist() == [2, 0, 0, 1, 1]
    run_cycled(w, a, b, sample, w.lean(), n)


def test_a_launch_without_a_tile(cuts):
    """the same 2^22 intervals followed by five empty ones: the second launch has no tile and starts no kernel; its cells are zero, its p NaN"""
    w, a, b = cuts
    tail = [(0, 7, 7), (1, 0, 0), (0, w.n, w.n + 3), (1, 50, 50), (0, 0, 0)]
    _, which, nt = cycled(w, w.lean(), CHUNK, tail)
    assert launch_cuts(nt) == [0, CHUNK, CHUNK + 5] and not nt[CHUNK:].any()
    sums, p = run_cycled(w, a, b, "pair", w.lean(), CHUNK, tail)      # (the head is compared there, cell by cell)
    assert not sums[CHUNK:].any() and np.isnan(p[CHUNK:]).all() and sums[:CHUNK, 0].any()


def test_cut_by_tile_count(cuts):
    """2 050 copies of the whole long sequence, 2 049 tiles each: the first launch is full after 2 048 of them; three short intervals behind them"""
    w, a, b = cuts
    T, n = w.T, w.n
    ivs = [(0, 0, n)] * 2050 + [(0, T - 40, T + 40), (1, 0, 50), (0, CHUNK - 1, CHUNK + 1)]
    nt = n_tiles(clipped_lengths(w.lens, *arrays(ivs)), T)
    assert int(nt[0]) == 2049 and launch_cuts(nt) == [0, 2048, 2053] and is_wide(nt[:2048]) and is_wide(nt[2048:])
    want = U.interval_sums(w.rows, w.lens, ivs[-4:])
    want = [want[0]] * 2050 + want[1:]
    assert want[0][0] == len(w.rows[0]) and want[-1][0] == 2 and want[-2][0] == len(w.rows[1]) and want[-3][0] > 2
    sums, p = a.diff_regions(b, *arrays(ivs))
    assert sums.tolist() == want
    assert all(small_support(s) for s in want[-3:]) and distinct_small(want[-3:]) == 3      # the three short ones are held to the exact model
    assert check_p(want, p) >= 3
    again = a.diff_regions(b, *arrays(ivs))
    assert sums.tobytes() == again[0].tobytes() and p.tobytes() == again[1].tobytes()
    single = single_sample_sums(a, w.lens, ivs[-4:])
    assert a.regions(*arrays(ivs)).tolist() == [single[0]] * 2050 + single[1:] and single[0][0] > want[0][0]


def bin_text(w, a, b, width):
    """the bin file of that width from bsx_meth_diff_regions on the same intervals, a call per sequence (as test_gpu_methdiff.py::test_bin_file)"""
    text, n = [D.BIN_HEADER], 0
    for c in a.write_order():
        start = np.arange(0, w.lens[c], width, dtype=np.int64)
        end = np.minimum(start + width, w.lens[c])
        sums, p = a.diff_regions(b, np.full(len(start), c, np.uint32), start, end)
        for j in np.nonzero(sums[:, 0])[0].tolist():
            text.append(D.interval_row_text(w.NAMES[c], int(start[j]), int(end[j]), None, sums[j].tolist(), float(p[j])))
            n += 1
    return "".join(text), n


def test_bin_file_across_its_chunk(cuts, tmp_path):
    """width 1: 2^22 + 77 bins on the long sequence, the last 77 in a second call; every common site is the bin [x, x + 1) with N = 1, its counts and the row's own p"""
    w, a, b = cuts
    want, n = [D.BIN_HEADER], 0
    for c in a.write_order():
        pos, counts, p = a.diff_report(b, c)
        assert [(x,) + tuple(q) for x, q in zip(pos.tolist(), counts.tolist())] == w.rows[c]
        want += [D.interval_row_text(w.NAMES[c], x, x + 1, None, [1] + q, px) for x, q, px in zip(pos.tolist(), counts.tolist(), p.tolist())]
        n += len(pos)
    want = "".join(want)
    for x in (CHUNK - 1, CHUNK, w.n - 1):          # rows on both sides of bin number 2^22, and the last position
        assert "cz_long\t%d\t%d\t1\t" % (x, x + 1) in want
    assert a.write_diff_bins(b, tmp_path / "b1.txt", 1) == n and U.read_text(tmp_path / "b1.txt") == want
    assert bin_text(w, a, b, 1) == (want, n)
    for width in (2, 4097, CHUNK):
        want, n = bin_text(w, a, b, width)
        assert a.write_diff_bins(b, tmp_path / "b.txt", width) == n and U.read_text(tmp_path / "b.txt") == want, width
        last = (w.n - 1) // width * width
        assert "cz_long\t%d\t%d\t" % (last, w.n) in want and "cz_long\t0\t%d\t" % width in want and 0 < want.index("\nca_short\t") < want.index("\ncz_long\t")
    assert want.count("\n") == 4 and "cz_long\t%d\t%d\t" % (CHUNK, CHUNK + 77) in want     # at 2^22 two bins on the long sequence, the second 77 long
