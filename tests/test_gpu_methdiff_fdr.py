"""q-values over all rows and de novo DMRs of the two-sample report on the GPU (bsx_meth_bh, bsx_meth_diff_report_all / _fetch_all, bsx_meth_diff_dmrs /
_fetch_dmrs, bsx_meth_write_diff_fdr / _write_diff_regions_fdr / _write_dmrs, the Meth methods over them and the new options of python -m
bsmap_amd.methdiff).

Nothing here has a tolerance.  q is compared bit for bit with the numpy model of fdr_model.py on the device's own p; the store is compared with the
per-sequence report that tests/test_gpu_methdiff.py pins; the DMRs are compared with the run model in Python integers on the fetched store, and their
sums and p with bsx_meth_diff_regions on the same spans."""
import os
import subprocess
import sys

import numpy as np
import pytest

import diff_model as D
import fdr_model as F
import meth_util as U
from bsmap_amd import BsxError
from bsmap_amd.methratio import Meth, bh

pytestmark = pytest.mark.gpu
BSX_ERR_ARG, BSX_ERR_STATE = -1, -5
STRANDS = ("++", "-+", "+-", "--")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def code_of(call):
    with pytest.raises(BsxError) as e:
        call()
    return e.value.code


# ---- 1. the core: q of p ------------------------------------------------------------------------------------------------------------------------
def bh_inputs(n):
    """two inputs of n values: heavy ties (20 values, zeros, ones, a denormal) with NaNs scattered through, and n distinct values"""
    rng = np.random.default_rng(1000 + n)
    pool = np.concatenate([rng.random(20), [0.0, 1.0, 5e-324]])
    tied = rng.choice(pool, n)
    tied[rng.random(n) < 0.1] = np.nan
    if n >= 5:
        tied[[0, n // 2, n - 1]] = [np.nan, 0.0, 5e-324]
    return tied, rng.permutation(n).astype(np.float64) / max(n, 1)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1024, 1025, 70001])
def test_bh_equals_the_model_bit_for_bit(n):
    for p in bh_inputs(n):
        q, again = bh(p), bh(p)
        assert q.dtype == np.float64 and q.shape == (n,)
        assert np.array_equal(np.isnan(q), np.isnan(p))                       # NaN in, NaN out, and nowhere else
        assert np.array_equal(bits(q), bits(F.bh(p)))
        assert np.array_equal(bits(q), bits(again))                           # two calls, the same bits
    if n == 1:
        assert np.isnan(bh([np.nan])[0]) and bh([0.3])[0] == 0.3
    if n == 70001:
        tied = bh_inputs(n)[0]
        assert 0.05 * n < np.isnan(tied).sum() < 0.15 * n and len(set(tied[~np.isnan(tied)].tolist())) == 23


def test_bh_rejects_what_is_no_probability():
    for bad in ([0.5, 1.5], [-0.1], [np.inf]):
        assert code_of(lambda: bh(bad)) == BSX_ERR_ARG


# ---- 2. the store on a world of reads -----------------------------------------------------------------------------------------------------------
class World:
    """Three sequences, named so that the sorted order is not the id order: 1 100 nt, 5 000 nt and 64 nt; random ACGT, reads of 30-60 nt on all four strands,
    each sample with its own methylation level.  The third sequence is covered in A only: no common site there."""
    NAMES = ["wc_short", "wa_long", "wb_a_only"]

    def __init__(self, tmp):
        rng = np.random.default_rng(59)
        self.refs = ["".join(rng.choice(list("ACGT"), n).tolist()) for n in (1100, 5000, 64)]
        self.lens = [len(r) for r in self.refs]
        self.fa = U.write_fasta(tmp / "world.fa", self.NAMES, self.refs)
        self.alns = [self.reads(rng, 0.8, True), self.reads(rng, 0.3, False)]

    def read(self, rng, c, pos, n, st, level):
        match, convert = ("C", "T") if st % 2 == 0 else ("G", "A")
        return (c, pos, st, 0, -1, "".join(convert if x == match and rng.random() >= level else x for x in self.refs[c][pos:pos + n]))

    def reads(self, rng, level, is_a):
        out = []
        for c, n in enumerate(self.lens[:2]):
            for _ in range(n // 2):
                k = int(rng.integers(30, 61))
                out.append(self.read(rng, c, int(rng.integers(0, n - k + 1)), k, int(rng.integers(0, 4)), level))
        if is_a:
            out += [self.read(rng, 2, 0, 64, st, level) for st in (0, 1, 0, 1)]
        return out

    def pair(self):
        """(a, b) with the samples piled up; the caller closes them"""
        a, b = Meth.from_fasta(self.fa), Meth.from_fasta(self.fa)
        for m, alns in zip((a, b), self.alns):
            m.add(alns, 0)
        return a, b


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("methdiff_fdr"))


@pytest.fixture(scope="module")
def both(world):
    a, b = world.pair()
    yield a, b
    a.close()
    b.close()


def concatenated(a, b, md):
    """the store's model: diff_report of every sequence at permille 0, in the writer's order"""
    order = a.write_order()
    per = [a.diff_report(b, c, md, 0) for c in order]
    row_start = np.cumsum([0] + [len(x[0]) for x in per]).astype(np.uint32)
    return order, row_start, np.concatenate([x[0] for x in per]), np.concatenate([x[1] for x in per]), np.concatenate([x[2] for x in per])


@pytest.mark.parametrize("md", [1, 3])
def test_store_is_every_sequence_report_and_q_over_all_rows(world, both, md):
    a, b = both
    assert a.write_order() == [1, 2, 0]                                          # sorted names: not the id order
    order, row_start, pos, counts, p = concatenated(a, b, md)
    before = a.diff_report(b, 0, md, 250)                                        # rows of the per-sequence buffers, to be found again below
    got = a.diff_report_all(b, md)
    assert [x.dtype for x in got] == [np.uint32, np.uint32, np.uint32, np.uint8, np.float64, np.float64]
    assert got[0].tolist() == row_start.tolist() and np.array_equal(got[1], pos) and np.array_equal(got[2], counts) and np.array_equal(bits(got[4]), bits(p))
    assert np.array_equal(bits(got[5]), bits(F.bh(got[4])))
    if md == 1:
        assert len(pos) >= 1025 and row_start[1] == row_start[2] and row_start[1] > 1024 and row_start[3] - row_start[2] > 100   # the A-only sequence has no row
    cls = np.concatenate([[D.context_class(world.refs[c], x) | (0 if world.refs[c][x] == "C" else 4) for x in pos[row_start[k]:row_start[k + 1]].tolist()]
                          for k, c in enumerate(order)]).astype(np.uint8)
    assert np.array_equal(got[3], cls)
    again = a.diff_report_all(b, md)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))           # two calls, the same bytes
    kept = (np.zeros(len(before[0]), np.uint32), np.zeros((len(before[0]), 4), np.uint32), np.zeros(len(before[0]), np.float64))
    a._call("bsx_meth_diff_fetch_rows", *[x.ctypes.data for x in kept])          # the store lives beside the rows of diff_report, not in their place
    assert len(before[0]) > 0 and all(x.tobytes() == y.tobytes() for x, y in zip(before, kept))


def test_store_of_a_sample_with_itself_and_errors(world, both):
    a, b = both
    row_start, pos, counts, cls, p, q = a.diff_report_all(a)
    assert len(p) > 1025 and np.all(p == 1.0) and np.all(q == 1.0) and np.array_equal(counts[:, :2], counts[:, 2:])
    with Meth.from_fasta(world.fa) as snp:
        snp.set_ct_snp(1)
        assert code_of(lambda: a.diff_report_all(snp)) == BSX_ERR_STATE and code_of(lambda: snp.diff_report_all(a)) == BSX_ERR_STATE
        assert code_of(lambda: a.write_dmrs(snp, "no-such-dir/x.txt")) == BSX_ERR_STATE
    with Meth.from_lengths([1100, 5000, 65]) as other, Meth.from_lengths(world.lens[:2]) as fewer:
        for y in (other, fewer):
            assert code_of(lambda: a.diff_report_all(y)) == BSX_ERR_ARG and code_of(lambda: a.diff_dmrs(y, 0.05)) == BSX_ERR_ARG
        assert code_of(lambda: other.write_diff(other, "no-such-dir/x.txt", fdr=True)) == BSX_ERR_ARG   # no names
        assert other.write_order() == [0, 1, 2] and other.diff_report_all(other)[0].tolist() == [0, 0, 0, 0]
        assert all(len(x) == 0 for x in other.diff_dmrs(other, 1.0, min_sites=1))
    for bad in (dict(max_q=1.5), dict(max_q=0.05, min_sites=0), dict(max_q=0.05, min_delta_permille=1001)):
        assert code_of(lambda: a.diff_dmrs(a, **bad)) == BSX_ERR_ARG
    for bad in (dict(max_q=1.5), dict(max_q=float("nan")), dict(max_q=-0.1), dict(max_p=float("nan"), fdr=True), dict(max_p=2.0, max_q=0.5)):
        assert code_of(lambda: a.write_diff(a, "no-such-dir/x.txt", **bad)) == BSX_ERR_ARG   # the limits of the q-value writer, as those of the DMR calls


def test_dmrs_need_the_store_of_their_pair(world):
    a, b = world.pair()
    try:
        assert code_of(lambda: a.diff_dmrs(b, 0.05)) == BSX_ERR_STATE           # before any report_all
        a.diff_report_all(b, 1)
        first = a.diff_dmrs(b, 0.9, min_sites=1)
        assert len(first[0]) > 0
        assert code_of(lambda: a.diff_dmrs(b, 0.9, min_depth=3)) == BSX_ERR_STATE   # another min_depth
        assert code_of(lambda: a.diff_dmrs(a, 0.9)) == BSX_ERR_STATE            # another sample B
        assert code_of(lambda: b.diff_dmrs(a, 0.9)) == BSX_ERR_STATE            # the store is A's
        assert all(x.tobytes() == y.tobytes() for x, y in zip(first, a.diff_dmrs(b, 0.9, min_sites=1)))
        b.add(world.alns[1][:1], 0)                                              # B's counters move: the store no longer stands for them
        assert code_of(lambda: a.diff_dmrs(b, 0.9)) == BSX_ERR_STATE
        a.diff_report_all(b, 1)
        assert len(a.diff_dmrs(b, 0.9, min_sites=1)[0]) > 0
    finally:
        a.close()
        b.close()


def test_a_sample_b_made_anew_is_another_sample(world, tmp_path):
    """One sample A against several samples B, each closed before the next is made over the same reference: the new handle may lie at the old one's
    address and have had as many adds, and is still another B.  The store of the first does not stand for it."""
    a = Meth.from_fasta(world.fa)
    try:
        a.add(world.alns[0], 0)
        b1 = Meth.from_fasta(world.fa)
        b1.add(world.alns[1], 0)
        a.diff_report_all(b1)
        first = a.diff_dmrs(b1, 0.9, min_sites=1)
        a.write_diff(b1, tmp_path / "one.txt", fdr=True)
        b1.close()
        made = []
        try:
            for _ in range(4):                                                   # several, kept alive: one of them is likely where b1 was
                made.append(Meth.from_fasta(world.fa))
                made[-1].add(world.alns[0], 0)                                   # other reads (A's own), one add as b1 had
            for b2 in made:
                assert code_of(lambda: a.diff_dmrs(b2, 0.9, min_sites=1)) == BSX_ERR_STATE
            b2 = made[0]
            rows = a.write_diff(b2, tmp_path / "two.txt", fdr=True)              # the writer builds a new store
            store = a.diff_report_all(b2)
            assert rows == len(store[4]) > 1025 and np.all(store[4] == 1.0) and np.all(store[5] == 1.0)   # A against its own reads
            assert U.read_text(tmp_path / "two.txt") != U.read_text(tmp_path / "one.txt")
            assert all(line.endswith("\t1.0000e+00\t1.0000e+00") for line in U.read_text(tmp_path / "two.txt").split("\n")[1:-1])
            assert len(first[0]) > 0 and len(a.diff_dmrs(b2, 0.9, min_sites=1)[0]) == 0
            assert a.write_dmrs(made[1], tmp_path / "dmr.txt", 0.9, 0, 300, 1) == 0   # likewise for the DMR writer: a store of its own pair
            assert code_of(lambda: a.diff_dmrs(b2, 0.9)) == BSX_ERR_STATE        # which is no longer b2's
        finally:
            for m in made:
                m.close()
    finally:
        a.close()


# ---- 3. DMRs on a planted world -----------------------------------------------------------------------------------------------------------------
A_ROW, B_ROW, NEUTRAL, WEAK = (8, 8, 0, 8), (0, 8, 8, 8), (4, 8, 4, 8), (12, 40, 30, 40)   # A fully methylated and B converted (sign -1), the reverse (+1), equal ratios,
#                                                                                           and a difference of 0.45 towards B that the delta rule at 500 leaves out
MAX_Q, PERMILLE, MAX_GAP, MIN_SITES = 0.01, 500, 30, 3


class Planted:
    """Cs in a text of As, each under one-letter reads: depth 8 in both samples (40 for the WEAK sites).  Sequence ids 1, 2, 0 are the store's order.  The first
    has three A_ROW sites at 40, 50, 60; the second starts with three at 70, 80, 90 (another sequence, numerically inside the gap) and then holds, with
    NEUTRAL sites in between: a run over store rows 255 / 256 that goes on after a gap of exactly MAX_GAP, one behind a gap of MAX_GAP + 1, a B_ROW run
    right behind it (the sign flips inside the gap), a run with a NEUTRAL site inside, a run of two, three WEAK sites, a run over store rows 1 023 / 1 024, and a
    run of 1 100 sites that holds candidates 255 / 256 and 1 023 / 1 024; the third sequence has a short B_ROW run."""
    NAMES = ["dm_c", "dm_a", "dm_b"]

    def __init__(self, tmp):
        big, at = [], [70 - 10]

        def put(counts, n=1, gap=10):
            for k in range(n):
                at[0] += gap if k == 0 else 10
                big.append((at[0], counts))

        put(A_ROW, 3)
        put(NEUTRAL, 244, 100)
        put(A_ROW, 12, 100)
        put(A_ROW, 5, MAX_GAP)
        put(A_ROW, 4, MAX_GAP + 1)
        put(B_ROW, 5)
        put(A_ROW, 2, 100); put(NEUTRAL); put(A_ROW, 2)
        put(A_ROW, 2, 100)
        put(WEAK, 3, 100)
        put(NEUTRAL, 730, 100)
        put(B_ROW, 20, 100)
        put(NEUTRAL, 5, 100)
        put(A_ROW, 1100, 100)
        put(NEUTRAL, 3, 100)
        self.sites = {1: [(40, A_ROW), (50, A_ROW), (60, A_ROW)], 2: big, 0: [(5, B_ROW), (15, B_ROW), (25, B_ROW), (35, NEUTRAL)]}
        self.lens = [64, 64, big[-1][0] + 16]
        refs = []
        for c in range(3):
            s = ["A"] * self.lens[c]
            for x, _ in self.sites[c]:
                s[x] = "C"
            refs.append("".join(s))
        self.fa = U.write_fasta(tmp / "planted.fa", self.NAMES, refs)

    def sample(self, which):
        """a handle where every site carries its (m, d) of sample `which` (0: A, 1: B) as one-letter reads"""
        flat = [(c, x, q[2 * which], q[2 * which + 1]) for c in range(3) for x, q in self.sites[c]]
        ds, ms = np.array([f[3] for f in flat], np.int64), np.array([f[2] for f in flat], np.int64)
        chr, pos = np.repeat([f[0] for f in flat], ds).astype(np.uint32), np.repeat([f[1] for f in flat], ds).astype(np.int64)
        first = np.repeat(np.cumsum(ds) - ds, ds)
        letters = np.where(np.arange(len(pos)) - first < np.repeat(ms, ds), ord("C"), ord("T")).astype(np.uint8)
        n = len(pos)
        m = Meth.from_fasta(self.fa)
        m.add_arrays(n, chr, pos, np.zeros(n, np.uint8), np.zeros(n, np.int32), np.full(n, -1, np.int64), np.append(letters, 0).astype(np.uint8),
                     np.arange(n + 1, dtype=np.uint64), 0)
        return m


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    w = Planted(tmp_path_factory.mktemp("planted"))
    a, b = w.sample(0), w.sample(1)
    store = a.diff_report_all(b)
    order = a.write_order()
    rows = [(order[k], int(x)) + tuple(int(v) for v in q4) for k in range(3) for x, q4 in zip(store[1][store[0][k]:store[0][k + 1]].tolist(), store[2][store[0][k]:store[0][k + 1]].tolist())]
    yield w, a, b, rows, store[5]
    a.close()
    b.close()


def device_dmrs(a, b, *args, **kw):
    chr, start, end, n_sig, sums, p = a.diff_dmrs(b, *args, **kw)
    return list(zip(chr.tolist(), start.tolist(), end.tolist(), n_sig.tolist())), sums, p


def test_the_planted_world_is_what_it_says(planted):
    """the store holds the planted sites, and the model on it shows every case the comparison below is about"""
    w, a, b, rows, q = planted
    assert a.write_order() == [1, 2, 0] and rows == [(c, x) + counts for c in (1, 2, 0) for x, counts in w.sites[c]]
    cand = [i for i, (r, qi) in enumerate(zip(rows, q)) if F.is_candidate(r, float(qi), MAX_Q, PERMILLE)]
    assert cand == [i for i, r in enumerate(rows) if r[2:] in (A_ROW, B_ROW)] and len(cand) > 1100     # max_q picks the planted sites and no other
    assert float(q.min()) > 1e-6                                                 # a max_q below every q exists
    runs = F.candidate_runs(rows, q, MAX_Q, PERMILLE, MAX_GAP)
    nth = {i: k for k, i in enumerate(cand)}                                     # store row -> its number among the candidates
    inside = lambda r: [rows[i][1] - rows[j][1] for i, j in zip(r[1:], r)]       # the gaps inside a run
    assert any(MAX_GAP in inside(r) for r in runs)                               # a gap of exactly max_gap joins
    nxt = list(zip(runs, runs[1:]))
    sgn = lambda r: F.sign(*rows[r[0]][2:])
    assert any(rows[s[0]][0] == rows[r[-1]][0] and sgn(r) == sgn(s) and rows[s[0]][1] - rows[r[-1]][1] == MAX_GAP + 1 for r, s in nxt)   # max_gap + 1 splits
    assert any(rows[s[0]][0] == rows[r[-1]][0] and sgn(r) != sgn(s) and 0 < rows[s[0]][1] - rows[r[-1]][1] <= MAX_GAP for r, s in nxt)   # a sign flip inside a gap
    assert any(rows[s[0]][0] != rows[r[-1]][0] and sgn(r) == sgn(s) and 0 <= rows[s[0]][1] - rows[r[-1]][1] <= MAX_GAP for r, s in nxt)  # the next sequence, within the gap
    assert any(r[-1] - r[0] + 1 > len(r) for r in runs)                          # a common site that is no candidate inside a run: N > n_sig
    assert any(len(r) < MIN_SITES for r in runs)                                 # a run that min_sites drops
    for edge in (256, 1024):
        assert any(r[0] < edge <= r[-1] for r in runs)                           # a run over a block border of the store's rows
        assert any(nth[r[0]] < edge <= nth[r[-1]] for r in runs)                 # and of the candidates
    assert any(F.is_candidate(r, float(qi), MAX_Q, 0) and not F.is_candidate(r, float(qi), MAX_Q, PERMILLE) for r, qi in zip(rows, q))   # what only the delta rule leaves out


PARAMS = [(MAX_Q, PERMILLE, MAX_GAP, MIN_SITES), (MAX_Q, PERMILLE, MAX_GAP, 1), (MAX_Q, 0, MAX_GAP, MIN_SITES), (MAX_Q, PERMILLE, MAX_GAP + 1, MIN_SITES),
          (MAX_Q, PERMILLE, 0, 1), (MAX_Q, PERMILLE, 9, 1), (1.0, 0, 10, 2), (MAX_Q, 1000, 100, 2), (MAX_Q, PERMILLE, 0xFFFFFFFF, 1)]


@pytest.mark.parametrize("max_q,permille,max_gap,min_sites", PARAMS)
def test_dmrs_equal_the_model_on_the_fetched_store(planted, max_q, permille, max_gap, min_sites):
    w, a, b, rows, q = planted
    want = F.dmrs(rows, q, max_q, permille, max_gap, min_sites)
    got, sums, p = device_dmrs(a, b, max_q, permille, max_gap, min_sites)
    assert got == want and len(want) > 0
    ref_sums, ref_p = a.diff_regions(b, [r[0] for r in want], [r[1] for r in want], [r[2] for r in want])
    assert sums.tobytes() == ref_sums.tobytes() and p.tobytes() == ref_p.tobytes()
    assert np.all(sums[:, 0] >= np.array([r[3] for r in want], np.uint64))
    if (max_q, permille, max_gap, min_sites) == PARAMS[0]:
        assert (2, 70, 91, 3) in got and (1, 40, 61, 3) in got and (0, 5, 26, 3) in got and any(r[3] == 17 for r in got) and any(r[3] == 1100 for r in got)
        assert any(int(s[0]) > r[3] for s, r in zip(sums, got)) and len(got) == len(F.dmrs(rows, q, max_q, permille, max_gap, 1)) - 1
    if max_gap == 0:
        assert len(got) > 1100 and all(r[3] == 1 and r[2] == r[1] + 1 for r in got)   # every candidate its own run: more runs than one block of them


def test_no_candidate_no_dmr_and_a_header_only_file(planted, tmp_path):
    w, a, b, rows, q = planted
    low = float(q.min()) / 2
    assert F.dmrs(rows, q, low, 0, MAX_GAP, 1) == [] and device_dmrs(a, b, low, 0, MAX_GAP, 1)[0] == []
    assert a.write_dmrs(b, tmp_path / "none.txt", low, 0, MAX_GAP, 1) == 0 and U.read_text(tmp_path / "none.txt") == F.DMR_HEADER
    assert a.write_diff(b, tmp_path / "noq.txt", max_q=low) == 0 and U.read_text(tmp_path / "noq.txt") == F.POS_FDR_HEADER


def test_dmr_file(planted, tmp_path):
    w, a, b, rows, q = planted
    for args in (PARAMS[0], PARAMS[2]):
        got, sums, p = device_dmrs(a, b, *args)
        want = F.DMR_HEADER + "".join(F.dmr_row_text(w.NAMES[r[0]], r[1], r[2], r[3], s, px) for r, s, px in zip(got, sums.tolist(), p.tolist()))
        assert a.write_dmrs(b, tmp_path / "dmr.txt", *args) == len(got) > 5 and U.read_text(tmp_path / "dmr.txt") == want
    assert "dm_b\t70\t91\t3\t3\t24\t24\t1.000\t0\t24\t0.000\t-1.000\t" in want
    with Meth.from_fasta(w.fa) as fresh:                                         # without a store the writer builds it
        assert fresh.write_dmrs(fresh, tmp_path / "self.txt", 1.0, 0, 300, 1) == 0 and U.read_text(tmp_path / "self.txt") == F.DMR_HEADER


# ---- 4. the files with q ------------------------------------------------------------------------------------------------------------------------
def test_position_file_with_q(world, both, tmp_path):
    a, b = both
    for md, permille, max_p in ((1, 0, None), (3, 200, None), (1, 0, 0.05), (1, 300, 0.2)):
        row_start, pos, counts, cls, p, q = a.diff_report_all(b, md)
        plain_n = a.write_diff(b, tmp_path / "plain.txt", md, permille, max_p)
        plain = U.read_text(tmp_path / "plain.txt").split("\n")[:-1]
        kept = [i for i in range(len(p)) if D.delta_keeps(*counts[i].tolist(), permille) and (max_p is None or p[i] <= max_p)]
        assert len(kept) == plain_n == len(plain) - 1 > 20
        limits = [None] + ([float(np.median(q[kept])), 0.0, 1.0] if max_p is None else [])
        for max_q in limits:
            n = a.write_diff(b, tmp_path / "fdr.txt", md, permille, max_p, max_q, fdr=True)
            want = [plain[0] + "\tq"] + [line + "\t%.4e" % q[i] for line, i in zip(plain[1:], kept) if max_q is None or q[i] <= max_q]
            assert U.read_text(tmp_path / "fdr.txt") == "".join(x + "\n" for x in want) and n == len(want) - 1
            if max_q is not None and 0.0 < max_q < 1.0:
                assert 0 < n < plain_n                                           # max_q filters rows and changes no printed q
                assert a.write_diff(b, tmp_path / "fdr2.txt", md, permille, max_p, max_q) == n and U.read_text(tmp_path / "fdr2.txt") == U.read_text(tmp_path / "fdr.txt")
    every = dict(x.rsplit("\t", 1) for x in U.read_text(tmp_path / "fdr.txt").split("\n")[1:-1])   # the last file: md 1, permille 300
    a.write_diff(b, tmp_path / "all.txt", 1, 0, fdr=True)
    unfiltered = dict(x.rsplit("\t", 1) for x in U.read_text(tmp_path / "all.txt").split("\n")[1:-1])
    assert 0 < len(every) < len(unfiltered) and all(unfiltered[k] == v for k, v in every.items())     # --min-delta leaves every printed q as it was


def test_region_file_with_q(world, both, tmp_path):
    a, b = both
    bed = tmp_path / "t.bed"
    open(bed, "w").write("wa_long\t100\t300\tfirst\nwa_long\t10\t4800\nwb_a_only\t0\t64\tnone\nwc_short\t1000\t99999\tclipped\nwa_long\t50\t50\nwa_long\t2000\t2040\tlast\n")
    recs = [(1, 100, 300, "first"), (1, 10, 4800, "."), (2, 0, 64, "none"), (0, 1000, 1100, "clipped"), (1, 50, 50, "."), (1, 2000, 2040, "last")]
    sums, p = a.diff_regions(b, *[[r[k] for r in recs] for k in range(3)])
    q = F.bh(p)
    assert np.isnan(p).sum() == 2 and np.array_equal(np.isnan(q), np.isnan(p)) and np.array_equal(bits(q), bits(bh(p)))
    want = F.REGION_FDR_HEADER + "".join(F.with_q(D.interval_row_text(world.NAMES[c], s, e, label, row, px), qx)
                                         for (c, s, e, label), row, px, qx in zip(recs, sums.tolist(), p.tolist(), q.tolist()))
    assert a.write_diff_regions(b, bed, tmp_path / "r.txt", fdr=True) == (6, 0) and U.read_text(tmp_path / "r.txt") == want
    assert "wb_a_only\t0\t64\tnone\t0\t0\t0\tNA\t0\t0\tNA\tNA\tNA\tNA\n" in want
    a.write_diff_regions(b, bed, tmp_path / "plain.txt")
    assert [x.rsplit("\t", 1)[0] for x in want.split("\n")[:-1]] == U.read_text(tmp_path / "plain.txt").split("\n")[:-1]


# ---- 5. the command line ------------------------------------------------------------------------------------------------------------------------
def test_command_line(world, both, tmp_path):
    a, b = both
    files = []
    for k, alns in enumerate(world.alns):
        files.append(str(tmp_path / ("s%d.bsp" % k)))
        with open(files[-1], "w") as f:
            f.write("".join("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t%d\n" % (i, s, "I" * len(s), world.NAMES[c], pos + 1, STRANDS[st], ins) for i, (c, pos, st, ins, _, s) in enumerate(alns)))
    bed = str(tmp_path / "t.bed")
    open(bed, "w").write("wa_long\t100\t300\tfirst\nwc_short\t0\t1100\nwb_a_only\t0\t64\n")

    def cli(tag, extra, dmr):
        out = [str(tmp_path / (tag + n)) for n in ("d.txt", "r.txt") + (("m.txt",) if dmr else ())]
        r = subprocess.run([sys.executable, "-m", "bsmap_amd.methdiff", "-q", "-t", "0", "-d", world.fa, "-o", out[0], "--a", files[0], "--b", files[1], "--regions", bed,
                            "--region-out", out[1], "--min-delta", "0.2", *(("--dmr-out", out[2]) if dmr else ()), *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout, [U.read_text(p) for p in out]

    common = len(a.diff_report_all(b)[4])
    head = "total %d valid mappings in a, %d in b, %d common cytosines, " % (len(world.alns[0]), len(world.alns[1]), common)
    want = [str(tmp_path / n) for n in ("wd.txt", "wr.txt", "wm.txt")]
    stdout, texts = cli("new", ("--max-q", "0.3", "--dmr-max-q", "0.9", "--dmr-max-gap", "40", "--dmr-min-sites", "2"), True)
    rows = a.write_diff(b, want[0], 1, 200, None, 0.3)
    a.write_diff_regions(b, bed, want[1], fdr=True)
    n_dmr = a.write_dmrs(b, want[2], 0.9, 200, 40, 2)
    assert texts == [U.read_text(p) for p in want] and texts[0].startswith(F.POS_FDR_HEADER) and texts[1].startswith(F.REGION_FDR_HEADER)
    assert stdout == head + "%d rows written, %d DMRs written.\n" % (rows, n_dmr) and 0 < rows < common and n_dmr > 0
    # Without the new options: the files and the line of before.  "Before" is held here as the plain writers of this same build and the old headers, not
    # as recorded bytes; what pins the old format itself is tests/test_gpu_methdiff.py, which this change leaves as it was.
    stdout, texts = cli("old", (), False)
    rows = a.write_diff(b, want[0], 1, 200)
    a.write_diff_regions(b, bed, want[1])
    assert texts == [U.read_text(p) for p in want[:2]] and texts[0].startswith(D.POS_HEADER) and texts[1].startswith(D.REGION_HEADER)
    assert stdout == head + "%d rows written.\n" % rows
