"""Two-sample differential methylation on the GPU (bsx_meth_diff_report_chr / _diff_regions / _write_diff / _write_diff_regions / _write_diff_bins, the Meth
methods over them and python -m bsmap_amd.methdiff).

Integers are compared exactly against code that is pinned elsewhere: the rows are the join on position of a.report() and b.report() followed by the delta
filter in Python integers, the interval sums are Python sums of those rows.  p is compared with the exact model of diff_model.py (math.comb and Fractions)
under the derived bound rtol = 64 (s + 16) 2^-53 for a support of s tables while the exact p is 1e-290 or more, and has to lie in [0, 1e-289] below that; a
case where some w(x) / w(mA) lies within 1e-8 of the selection limit without being equal to it is left out, and at most 1 % of the cases may be."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import diff_model as D
import meth_util as U
from bsmap_amd import BsxError
from bsmap_amd.methratio import Meth

pytestmark = pytest.mark.gpu
BSX_ERR_ARG, BSX_ERR_IO, BSX_ERR_STATE = -1, -2, -5
STRANDS = ("++", "-+", "+-", "--")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the worlds ----------------------------------------------------------------------------------------------------------------------------------
class World:
    """Three sequences, named so that the sorted order is not the id order: 1 100 nt, 5 000 nt and 64 nt.  Random ACGT with a C or G planted at items 255 / 256
    and 1 023 / 1 024 of a compaction block, at both sides of a tile border (2 047 / 2 048), at the last position of the first sequence and the first of the
    second.  Reads of 30-60 nt on all four strands, each sample with its own methylation level, and reads that reach both ends of the first two sequences.
    The third sequence is covered in A only: no common site; positions 300-420 of the second likewise."""
    NAMES = ["wc_short", "wa_long", "wb_a_only"]

    def __init__(self, tmp):
        rng = np.random.default_rng(53)
        self.refs = []
        for n in (1100, 5000, 64):
            s = rng.choice(list("ACGT"), n).tolist()
            for at, letter in ((255, "C"), (256, "G"), (1023, "C"), (1024, "G"), (2047, "G"), (2048, "C"), (0, "G"), (n - 1, "C")):
                if at < n:
                    s[at] = letter
            self.refs.append("".join(s))
        self.lens = [len(r) for r in self.refs]
        self.fa = U.write_fasta(tmp / "world.fa", self.NAMES, self.refs)
        self.alns = [self.reads(rng, 0.7, True), self.reads(rng, 0.35, False)]

    def read(self, rng, c, pos, n, st, level):
        match, convert = ("C", "T") if st % 2 == 0 else ("G", "A")
        return (c, pos, st, 0, -1, "".join(convert if x == match and rng.random() >= level else x for x in self.refs[c][pos:pos + n]))

    def reads(self, rng, level, is_a):
        out = []
        for c, n in enumerate(self.lens[:2]):
            for _ in range(n // 6):
                k = int(rng.integers(30, 61))
                pos = int(rng.integers(0, n - k + 1))
                if not is_a and c == 1 and pos + k > 300 and pos < 420:
                    continue
                out.append(self.read(rng, c, pos, k, int(rng.integers(0, 4)), level))
            for st in (0, 1, 0, 1, 3, 2):   # both ends, both reference strands, three deep
                out += [self.read(rng, c, 0, 40, st, level), self.read(rng, c, n - 40, 40, st, level)]
            for at in (255, 1023, 2047):      # and the planted letters at the block and tile borders
                if at + 21 < n:
                    out += [self.read(rng, c, at - 19, 40, st, level) for st in (0, 1)]
        if is_a:
            out += [self.read(rng, 2, 0, 64, st, level) for st in (0, 1, 0, 1)]
        return out

    def pair(self, mask=0, cpg=False):
        """(a, b) with the samples piled up; the caller closes them"""
        a, b = Meth.from_fasta(self.fa), Meth.from_fasta(self.fa)
        for m, alns in zip((a, b), self.alns):
            m.set_contexts(mask)
            m.add(alns, 0)
            if cpg:
                m.combine_cpg()
        return a, b


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return World(tmp_path_factory.mktemp("methdiff"))


@pytest.fixture(scope="module")
def both(world):
    a, b = world.pair()
    yield a, b
    a.close()
    b.close()


def got_rows(a, b, c, min_depth=1, permille=0):
    pos, counts, p = a.diff_report(b, c, min_depth, permille)
    assert pos.dtype == np.uint32 and counts.shape == (len(pos), 4) and p.shape == (len(pos),) and p.dtype == np.float64
    return [(int(x),) + tuple(int(v) for v in row) for x, row in zip(pos, counts)], p


def check_p(ps, quads):
    left_out = [q for q in set(quads) if D.near_boundary(*q)]
    assert len(left_out) * 100 <= len(set(quads))
    errors = [e for e in (D.p_error(float(p), q) for p, q in zip(ps, quads) if q not in left_out) if e]
    assert not errors, errors[:10]


# ---- 1. integer columns against pinned code ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,cpg", [(0, False), (1, False), (0, True), (1, True)], ids=["all", "CG", "all-g", "CG-g"])
def test_rows_are_the_join_of_the_two_reports(world, mask, cpg):
    a, b = world.pair(mask, cpg)
    try:
        for md in (1, 3):
            for c in range(3):
                for permille in (0, 250, 1000):
                    want = U.joined(a, b, c, md, permille)
                    got, p = got_rows(a, b, c, md, permille)
                    assert got == want, (md, c, permille)
                    assert np.all((p >= 0) & (p <= 1))
            assert len(U.joined(a, b, 1, md)) > 50 and U.joined(a, b, 2, md) == [] and 0 < len(U.joined(a, b, 1, md, 250)) < len(U.joined(a, b, 1, md))
        if mask == 0 and not cpg:   # the planted rows: block and tile borders, the last position of a sequence and the first of the next
            pos0, pos1 = ({r[0] for r in U.joined(a, b, c, 1)} for c in (0, 1))
            assert {255, 256, 1023, 1024, 1099} <= pos0 and {0, 255, 256, 1023, 1024, 2047, 2048, 4999} <= pos1
            assert not any(300 <= x < 420 for x in pos1) and any(300 <= x < 420 for x in a.report(1)[0].tolist())   # covered in A only
    finally:
        a.close()
        b.close()


# ---- 2. p against the exact model ----------------------------------------------------------------------------------------------------------------
EXTRA = [(1, 2, 3, 4)]   # behind the directed and the seeded quadruples: the delta filter's own case


def stacked(fa, ms, ds):
    """a handle where the C at 8 i carries ms[i] methylated of ds[i] one-letter reads"""
    ms, ds = np.asarray(ms, np.int64), np.asarray(ds, np.int64)
    site = np.repeat(np.arange(len(ds)), ds)
    first = np.repeat(np.cumsum(ds) - ds, ds)
    letters = np.where(np.arange(len(site)) - first < np.repeat(ms, ds), ord("C"), ord("T")).astype(np.uint8)
    n = len(site)
    m = Meth.from_fasta(fa)
    m.add_arrays(n, np.zeros(n, np.uint32), site * 8, np.zeros(n, np.uint8), np.zeros(n, np.int32), np.full(n, -1, np.int64), np.append(letters, 0).astype(np.uint8),
                 np.arange(n + 1, dtype=np.uint64), 0)
    return m


@pytest.fixture(scope="module")
def iso(tmp_path_factory):
    seeded = D.cases()[:2992]
    quads = D.DIRECTED + [seeded[k * 2992 // 1000] for k in range(1000)] + EXTRA
    fa = U.write_fasta(tmp_path_factory.mktemp("iso") / "iso.fa", ["iso"], ["CAAAAAAA" * len(quads)])
    a, b = stacked(fa, [q[0] for q in quads], [q[1] for q in quads]), stacked(fa, [q[2] for q in quads], [q[3] for q in quads])
    yield a, b, quads
    a.close()
    b.close()


def test_p_keeps_the_bound(iso):
    a, b, quads = iso
    assert a.valid_mappings() == sum(q[1] for q in quads) and b.valid_mappings() == sum(q[3] for q in quads)
    rows, p = got_rows(a, b, 0)
    assert rows == [(8 * i,) + q for i, q in enumerate(quads)]
    check_p(p, quads)
    by = dict(zip(quads, p.tolist()))
    assert by[(0, 1, 0, 1)] == 1.0 and by[(5, 10, 5, 10)] == 1.0 and by[(1, 1, 0, 1)] == 1.0 and by[(3, 3, 0, 3)] == pytest.approx(0.1, rel=1e-13)
    assert 0.0 <= by[(0, 4000, 2500, 2500)] <= 1e-289 and 0.0 <= by[(4000, 4000, 0, 2500)] <= 1e-289
    rows, p = got_rows(a, a, 0)
    assert rows == [(8 * i, q[0], q[1], q[0], q[1]) for i, q in enumerate(quads)] and np.all(p == 1.0)


def test_delta_filter_at_its_limit(iso):
    a, b, quads = iso
    at = 8 * (len(quads) - 1)                          # 1/2 against 3/4: the ratios differ by exactly 250 per mille
    assert at in [r[0] for r in got_rows(a, b, 0, 1, 250)[0]] and at not in [r[0] for r in got_rows(a, b, 0, 1, 251)[0]]
    for permille in (1, 500, 999, 1000):
        assert got_rows(a, b, 0, 1, permille)[0] == [(8 * i,) + q for i, q in enumerate(quads) if D.delta_keeps(*q, permille)]


# ---- 3. the same bits twice ----------------------------------------------------------------------------------------------------------------------
INTERVALS = [(1, 100, 300), (1, 2000, 2100), (1, 10, 4800), (1, 50, 50), (1, 150, 400), (1, 100, 300), (1, 4900, 9999999), (2, 0, 64), (1, 300, 420), (0, 0, 1100),
             (1, 0, 5000), (0, 1099, 1100), (1, 2047, 2049), (1, 0, 1)]   # inside a tile, across a border, more than two tiles, zero length, overlapping, repeated,
#                                                                          end clipped, no common site (twice), whole sequences, single positions


def test_two_calls_give_the_same_bytes(both):
    a, b = both
    first, again = a.diff_report(b, 1), a.diff_report(b, 1)
    assert len(first[0]) > 300 and all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
    iv = [np.array([v[k] for v in INTERVALS], np.uint32) for k in range(3)]
    first, again = a.diff_regions(b, *iv), a.diff_regions(b, *iv)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))


# ---- 4. regions ----------------------------------------------------------------------------------------------------------------------------------
def check_interval_p(sums, p):
    for s, x in zip(sums, p.tolist()):
        assert math.isnan(x) if not s[0] else 0.0 <= x <= 1.0, (s, x)
    some = [(tuple(s[1:]), x) for s, x in zip(sums, p.tolist()) if s[0]]
    check_p([x for _, x in some], [q for q, _ in some])


@pytest.mark.parametrize("md", [1, 3])
def test_region_sums_and_p(world, both, md):
    a, b = both
    assert a.L.bsx_meth_region_tile() == 2048
    rows = [U.joined(a, b, c, md) for c in range(3)]
    sums, p = a.diff_regions(b, *[[v[k] for v in INTERVALS] for k in range(3)], md)
    want = U.interval_sums(rows, world.lens, INTERVALS)
    assert sums.dtype == np.uint64 and sums.tolist() == want
    assert want[0] == want[5] and want[3] == want[7] == want[8] == [0] * 5 and want[2][0] > 500 and want[9][0] == len(rows[0]) and want[11][0] == want[13][0] == 1
    check_interval_p(want, p)
    assert a.diff_regions(b, [], [], [])[0].shape == (0, 5)


# ---- 5. files ------------------------------------------------------------------------------------------------------------------------------------
def pos_text(world, a, b, md, permille, max_p=None):
    text, n = D.POS_HEADER, 0
    for c in sorted(range(3), key=lambda c: world.NAMES[c]):
        pos, counts, p = a.diff_report(b, c, md, permille)
        for x, q, px in zip(pos.tolist(), counts.tolist(), p.tolist()):
            if max_p is None or px <= max_p:
                text += D.pos_row_text(world.NAMES[c], x, world.refs[c][x], D.context_class(world.refs[c], x), q, px)
                n += 1
    return text, n


def test_position_file(world, both, tmp_path):
    a, b = both
    for md, permille in ((1, 0), (3, 200)):
        want, n = pos_text(world, a, b, md, permille)
        assert a.write_diff(b, tmp_path / "d.txt", md, permille) == n > 100 and U.read_text(tmp_path / "d.txt") == want
    ps = sorted(set(a.diff_report(b, 1)[2].tolist()))
    k = len(ps) // 3
    limit = (ps[k] + ps[k + 1]) / 2
    want, n = pos_text(world, a, b, 1, 0, limit)
    assert a.write_diff(b, tmp_path / "p.txt", 1, 0, limit) == n and 0 < n < len(a.diff_report(b, 0)[0]) + len(a.diff_report(b, 1)[0])
    assert U.read_text(tmp_path / "p.txt") == want
    assert a.write_diff(b, tmp_path / "none.txt", 1, 0, 0.0) == 0 and U.read_text(tmp_path / "none.txt") == D.POS_HEADER
    kinds = {line.split("\t")[3] for line in want.split("\n")[1:-1]}
    assert kinds >= {"CG", "CHG", "CHH"} and {line.split("\t")[2] for line in want.split("\n")[1:-1]} == {"+", "-"}


def test_region_file(world, both, tmp_path):
    a, b = both
    bed = tmp_path / "t.bed"
    open(bed, "w", newline="").write("# targets\nwa_long\t100\t300\tfirst\nwa_long 10 4800\nabsent\t0\t5\tgone\nwb_a_only\t0\t64\tnone\nwc_short\t1000\t99999\tclipped\r\nwa_long\t50\t50")
    recs = [(1, 100, 300, "first"), (1, 10, 4800, "."), (2, 0, 64, "none"), (0, 1000, 1100, "clipped"), (1, 50, 50, ".")]
    sums, p = a.diff_regions(b, *[[r[k] for r in recs] for k in range(3)])
    want = D.REGION_HEADER + "".join(D.interval_row_text(world.NAMES[c], s, e, label, row, px) for (c, s, e, label), row, px in zip(recs, sums.tolist(), p.tolist()))
    assert a.write_diff_regions(b, bed, tmp_path / "r.txt") == (5, 1) and U.read_text(tmp_path / "r.txt") == want
    assert "wb_a_only\t0\t64\tnone\t0\t0\t0\tNA\t0\t0\tNA\tNA\tNA\n" in want and want.count("NA") == 8
    open(bed, "w").write("wa_long\t0\t5\n\nwa_long\t9\t5\n")
    with pytest.raises(BsxError) as e:
        a.write_diff_regions(b, bed, tmp_path / "bad.txt")
    assert e.value.code == BSX_ERR_IO and "line 3" in str(e.value) and not os.path.exists(tmp_path / "bad.txt")


def test_bin_file(world, both, tmp_path):
    a, b = both
    want, n = D.BIN_HEADER, 0
    for c in sorted(range(3), key=lambda c: world.NAMES[c]):
        ivs = [(c, s, min(s + 100, world.lens[c])) for s in range(0, world.lens[c], 100)]
        sums, p = a.diff_regions(b, *[[v[k] for v in ivs] for k in range(3)])
        for (_, s, e), row, px in zip(ivs, sums.tolist(), p.tolist()):
            if row[0]:
                want += D.interval_row_text(world.NAMES[c], s, e, None, row, px)
                n += 1
    assert a.write_diff_bins(b, tmp_path / "b.txt", 100) == n and U.read_text(tmp_path / "b.txt") == want
    assert 55 <= n <= 11 + 50 - 1 and "wb_a_only" not in want and "wa_long\t300\t400\t" not in want and "wa_long\t4900\t5000\t" in want   # not the bin that B does not cover


# ---- 6. errors -----------------------------------------------------------------------------------------------------------------------------------
def code_of(call):
    with pytest.raises(BsxError) as e:
        call()
    return e.value.code


def test_errors(world, both, tmp_path):
    a, b = both
    one = np.zeros(8, np.uint32)
    calls = lambda x, y: (lambda: x.diff_report(y, 0), lambda: x.diff_regions(y, [0], [0], [10]), lambda: x.write_diff(y, tmp_path / "e.txt"),
                          lambda: x.write_diff_bins(y, tmp_path / "e.txt", 100))
    with Meth.from_lengths([1100, 5000, 65]) as other, Meth.from_lengths(world.lens[:2]) as fewer:
        for y in (other, fewer):
            assert [code_of(f) for f in calls(a, y)] == [BSX_ERR_ARG] * 4 and [code_of(f) for f in calls(y, a)][:2] == [BSX_ERR_ARG] * 2
    with Meth.from_fasta(world.fa) as masked:
        masked.set_contexts(1)
        assert [code_of(f) for f in calls(a, masked)] == [BSX_ERR_ARG] * 4
        masked.set_contexts(0)
        assert len(a.diff_report(masked, 0)[0]) == 0          # the same rule again: comparable, and nothing piled up in it
    with Meth.from_fasta(world.fa) as snp:
        snp.set_ct_snp(1)
        assert [code_of(f) for f in calls(a, snp)] == [BSX_ERR_STATE] * 4 and [code_of(f) for f in calls(snp, a)] == [BSX_ERR_STATE] * 4
    assert not os.path.exists(tmp_path / "e.txt")
    assert code_of(lambda: a.diff_report(b, 0, 1, 1001)) == BSX_ERR_ARG and code_of(lambda: a.write_diff(b, tmp_path / "e.txt", 1, 1001)) == BSX_ERR_ARG
    assert code_of(lambda: a.diff_report(b, 3)) == BSX_ERR_ARG and code_of(lambda: a.write_diff_bins(b, tmp_path / "e.txt", 0)) == BSX_ERR_ARG
    assert code_of(lambda: a.diff_regions(b, [3], [0], [1])) == BSX_ERR_ARG and code_of(lambda: a.diff_regions(b, [1], [5], [4])) == BSX_ERR_ARG
    assert a.L.bsx_meth_diff_regions(a.h, b.h, 1, None, one.ctypes.data, one.ctypes.data, 1, one.ctypes.data, one.ctypes.data) == BSX_ERR_ARG
    assert a.L.bsx_meth_diff_regions(a.h, b.h, 0, None, None, None, 1, None, None) == 0
    with Meth.from_lengths(world.lens) as nameless:
        assert code_of(lambda: nameless.write_diff(nameless, tmp_path / "e.txt")) == BSX_ERR_ARG and len(nameless.diff_report(nameless, 0)[0]) == 0
    assert not os.path.exists(tmp_path / "e.txt")
    with pytest.raises(ValueError, match="closed"):
        a.diff_report(nameless, 0)


# ---- 7. nothing else moved -----------------------------------------------------------------------------------------------------------------------
def test_the_diff_calls_change_nothing(world, tmp_path):
    a, b = Meth.from_fasta(world.fa), Meth.from_fasta(world.fa)
    try:
        for m, alns in zip((a, b), world.alns):
            m.set_pdr(2)
            m.set_epi()
            m.add(alns, 0)
        before = [U.written_table(m, tmp_path / "t.txt") for m in (a, b)]
        pdr, epi, rows = [x.tobytes() for x in a.pdr_report(1)], [x.tobytes() for x in a.epi_report(1)], [x.tobytes() for x in a.report(1)[:3]]
        a.diff_report(b, 1)
        a.diff_regions(b, [0, 1], [0, 0], [1100, 5000])
        a.write_diff(b, tmp_path / "d.txt", 1, 100, 0.5)
        open(tmp_path / "x.bed", "w").write("wa_long\t0\t5000\n")
        a.write_diff_regions(b, tmp_path / "x.bed", tmp_path / "r.txt")
        a.write_diff_bins(b, tmp_path / "b.txt", 250)
        nr = [np.zeros(n, np.uint32) for n in (len(pdr[0]) // 4,) * 3]
        a._call("bsx_meth_pdr_fetch_rows", *[x.ctypes.data for x in nr])           # the rows fetched before the diff calls are still there
        assert [x.tobytes() for x in nr] == pdr and len(pdr[0]) > 0
        pos0, counts = np.zeros((len(epi[0]) // 16, 4), np.uint32), np.zeros((len(epi[0]) // 16, 16), np.uint32)
        a._call("bsx_meth_epi_fetch_rows", pos0.ctypes.data, counts.ctypes.data)
        assert [pos0.tobytes(), counts.tobytes()] == epi and len(epi[0]) > 0
        last = [np.zeros(len(rows[0]) // 4, np.uint32) for _ in range(3)]
        a._call("bsx_meth_fetch_rows", *[x.ctypes.data for x in last])
        assert [x.tobytes() for x in last] == rows
        assert [U.written_table(m, tmp_path / "t.txt") for m in (a, b)] == before
        assert (a.valid_mappings(), b.valid_mappings()) == (len(world.alns[0]), len(world.alns[1]))
    finally:
        a.close()
        b.close()


# ---- 8. the command line -------------------------------------------------------------------------------------------------------------------------
def test_command_line(world, both, tmp_path):
    a, b = both
    files = []
    for k, alns in enumerate(world.alns):
        files.append(str(tmp_path / ("s%d.bsp" % k)))
        with open(files[-1], "w") as f:
            f.write("".join("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t%d\n" % (i, s, "I" * len(s), world.NAMES[c], pos + 1, STRANDS[st], ins) for i, (c, pos, st, ins, _, s) in enumerate(alns)))
    bed = str(tmp_path / "t.bed")
    open(bed, "w").write("wa_long\t100\t300\tfirst\nwc_short\t0\t1100\nwb_a_only\t0\t64\n")

    def cli(first, second, tag, extra=()):
        out = [str(tmp_path / (tag + n)) for n in ("d.txt", "r.txt", "b.txt")]
        r = subprocess.run([sys.executable, "-m", "bsmap_amd.methdiff", "-q", "-t", "0", "-d", world.fa, "-o", out[0], "--a", first, "--b", second, "--regions", bed,
                            "--region-out", out[1], "--bin", "100", "--bin-out", out[2], *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout, [U.read_text(p) for p in out]

    stdout, texts = cli(files[0], files[1], "ab")
    want = [str(tmp_path / n) for n in ("wd.txt", "wr.txt", "wb.txt")]
    rows = a.write_diff(b, want[0])
    a.write_diff_regions(b, bed, want[1])
    a.write_diff_bins(b, want[2], 100)
    assert texts == [U.read_text(p) for p in want]
    common = sum(len(a.diff_report(b, c)[0]) for c in range(3))
    assert stdout == "total %d valid mappings in a, %d in b, %d common cytosines, %d rows written.\n" % (len(world.alns[0]), len(world.alns[1]), common, rows) and rows == common
    _, swapped = cli(files[1], files[0], "ba")

    def columns(text):
        return [line.split("\t") for line in text.split("\n")[1:-1]]
    for x, y in zip(columns(texts[0]), columns(swapped[0])):
        assert x[:4] == y[:4] and x[4:7] == y[7:10] and x[7:10] == y[4:7] and x[11] == y[11]
        assert float(x[10]) == -float(y[10]) and (x[10][0] != y[10][0] or float(x[10]) == 0.0)
    assert len(columns(texts[0])) == len(columns(swapped[0])) == rows
    stdout, filtered = cli(files[0], files[1], "f", ("--min-delta", "0.25", "--max-p", "0.05", "-m", "3"))
    assert a.write_diff(b, want[0], 3, 250, 0.05) == int(stdout.split()[-3]) > 0 and filtered[0] == U.read_text(want[0])
