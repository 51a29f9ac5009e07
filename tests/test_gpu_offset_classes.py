"""k_hscan_same's groups that span offset classes: reads that walk one window with read offsets h and h + 32 d share one fetch and one shift of the candidates'
reference (hs_group: a frame d words longer, moved down a word where the rows of the next class begin).  Needs an MI355X.

The genome, and what its copies are, is that of tests/test_gpu_scan_word_order.py: 421 copies of one 200-letter unit whose index keys are all the unit's, so
every seed of a read made from the unit is one bucket of the 421 copies in position order — one full step of four chunks plus a partial one, with the copies
that are the unit itself at lanes 0 and 63 of a full chunk, lane 0 of the second step and the last lane of the partial chunk.  The heavy threshold is 48, so
those lists are deferred and scanned by k_hscan_same.

A read here is unit[a : a + L] with its C kept.  The seed at unit letter s lies at read letter s - a, so two reads of equal length that walk the bucket of one
seed do so with read offsets that differ by exactly the difference of their a.  But they have to walk it IN THE SAME PASS: a deferred read publishes its lists one
per pass, in the planner's order (smallest bucket first, equal buckets in segment order), and stops at the first list that yields a hit.  A pristine read's
buckets are all the copies', so its first list is the seed at its first letters — unit letter a — and reads of different a never meet; the same holds at -v 0,
where a read has one seed.  So the reads that are to meet carry one of their differences in each seed BEFORE the shared one (at letter 12 or 13 of the seed:
every 16-mer of that segment that can lie on the index grid holds it): those buckets are a handful of entries, come first in the planner's order and are walked
by the control pass itself, and the first list that goes to the scan kernel, in the first pass, is the shared seed's.  first_heavy_list works that out from the
oracle's plan for every read, and the test checks that the construction holds before it asks for anything.
  five words (129-160 letters; a group needs equal word count, not equal length): L = 144 with a = 0 and 32 meet — at -v 2 at unit letter 32 (two and no
          seeds spoiled), at -v 6 at letter 64 or the planner's start beside it (four and two) — with offsets 32 apart: one group of two classes.  L = 144,
          a = 16 walks their window with an offset 16 off theirs — the other value of the low five bits — and must stay out; a = 4 and 36, and L = 132 with
          a = 64, walk windows nearby.  Three classes in one window, and the split of a set that reaches further than a group spans, are the third test's;
  four words (L = 100, a = 0, 32, 64, 96, built to meet in the same way), in batches of their own: reads of 97-128 letters keep groups of one offset (C2 lost
          time with more), so these must NOT merge although they meet with offsets 32 apart: counter 15 stays 0 under the default.
Every batch holds ONE read per (L, a), so no two tasks of a batch have the same window, length and offset: with BSX_SAME_D=0 every group is one task, and
counter 15 (candidates evaluated in groups of two reads and more) must be 0.  With the default it must be above 0 in the batches where reads meet: those with v
and with v + 1 differences and the one with an N, at -v 2 and 6.  Where no two reads can meet — the pristine batches and all of -v 0 — counter 15 is not asked
to be above 0; everything else is asked of them too.
The batches of one -v: the reads pristine; with v differences (the spoiled seeds, the others in the read's last letters that can carry one), a hit of class v
wherever the pristine read has one; with v + 1: no hit, every list walked; and with v differences and an N in the last word (the evaluation with three
operations per word).  Records are compared with the oracle's unit by unit as tests/test_gpu_boundaries.py does, with the work counters off (the exiting
evaluation for five words) and on, counters 0-3 with the oracle's when counted, and the result bytes of BSX_SAME_D=0 with the default's.

The second case: 20 reads of a = 0 that differ in one C not kept (T under the genome's C is not counted: every one is a hit) and 6 of a = 32, L = 144, -v 2.
The 20 are more than HG_R = 16: a full group of one class, then a group in which rows of d = 0 are followed by rows of d = 1."""
import numpy as np
import pytest

import bsmap_amd as B
import bsx_testdata as td
import test_gpu_boundaries as GB
import test_gpu_scan_word_order as WO

pytestmark = pytest.mark.gpu

OFFSETS = {144: (0, 32, 4, 16, 36), 132: (64,), 100: (0, 32, 64, 96)}


def shared_seed(L, a, v):
    """the unit letter of the seed whose bucket is the read's first heavy list (see the module text)"""
    if L >= 129:
        return 36 if a in (4, 36) else 64 if v >= 6 or a == 64 else 32
    if v >= 6:
        return 96 if a else 32
    return 32 if a < 64 else 96


@pytest.fixture(scope="module")
def world():
    g, unit, copies, pos = WO.make_genome()
    return dict(fasta=td.fasta_text(g), unit=unit, copies=copies, pos=pos)


def _read(unit, L, a, n_subs=0, spoil=0, n_at=(), drop=(), tag=""):
    """unit[a : a + L] with its C kept; n_subs differences: one in each of the first `spoil` seeds (at letter 12 or 13 of the seed where that letter can carry one: inside every
    16-mer of that seed that can lie on the index grid, whatever start and phase the planner tries; else a few letters before — the oracle's plan is checked), the others in the read's last letters that can carry one"""
    u = unit[a:a + L]
    subs = []
    for j in range(spoil):
        c = [16 * j + k for k in (12, 13, 11, 10, 9, 8) if u[16 * j + k] in "GA"]
        assert c, (L, a, j)
        subs.append(c[0])
    assert len(subs) <= n_subs
    car = [i for i in WO._at(u, 0, L, "GA") if i not in n_at and i not in subs]
    subs += car[len(car) - (n_subs - len(subs)):] if n_subs > len(subs) else []
    seq = list(u)
    for i in range(L):
        if i in subs:
            seq[i] = "A" if u[i] == "G" else "G"
        elif i in n_at:
            seq[i] = "N"
        elif u[i] == "C" and i in drop:
            seq[i] = "T"
    seq = "".join(seq)
    assert sum(1 for i in range(L) if WO._counted(seq[i], u[i])) == n_subs
    return dict(name="L%d_a%d_%s" % (L, a, tag), seq=seq, qual="I" * L, L=L, a=a)


def first_heavy_list(r, unit, plan):
    """(unit letter, read offset h) of the first seed, in the planner's order, whose bucket is the copies': the phase of a segment reads the 16-mer at read letter
    16 seg + start + (0, 3, 2, 1)[phase], one of the four lies on the index grid (the copies stand at multiples of 4), and its bucket is the copies' if the read
    has the unit's letters there (C or T alike).  The lists before it are a handful of candidates each and are walked by the control pass itself"""
    starts, order = plan
    u = unit[r["a"]:r["a"] + r["L"]]
    for seg in order:
        for k in range(4):
            q = 16 * seg + starts[seg] + k
            if (r["a"] + q) % 4 == 0 and q + 16 <= r["L"] and all(x == y or (x, y) == ("T", "C") for x, y in zip(r["seq"][q:q + 16], u[q:q + 16])):
                return r["a"] + q, -q
    return None, 0


def make_batches(unit, v, five):
    """the batches of one -v and word count (five words, or the four-word reads on their own), one read per (L, a) each: (kind, reads, whether reads of
    the batch meet in one window in one pass)"""
    la = [(L, a) for L in sorted(OFFSETS, reverse=True) for a in OFFSETS[L] if (L >= 129) == five]
    out = [("pristine", [_read(unit, L, a, tag="pristine") for L, a in la], False)]
    if v:
        sp = lambda L, a: (shared_seed(L, a, v) - a) // 16
        out.append(("within", [_read(unit, L, a, v, sp(L, a), tag="within") for L, a in la], True))
        out.append(("over", [_read(unit, L, a, v + 1, sp(L, a), tag="over") for L, a in la], True))
        out.append(("N", [_read(unit, L, a, v, sp(L, a), n_at=(L - 2,), tag="N") for L, a in la], True))
    else:
        out.append(("over", [_read(unit, L, a, 1, tag="over") for L, a in la], False))
        out.append(("N", [_read(unit, L, a, n_at=(L - 2,), tag="N") for L, a in la], False))
    return out


def _run(gref, oracle, oref, kw, reads, monkeypatch, route, merges, grouped_without=False, settings=("0", None)):
    """one batch through the settings of BSX_SAME_D (None: the default) and both of the work counters, against the oracle; merges: reads of the batch meet in one
    window with offsets 32 d apart.  Returns the oracle's records and counter 15 by setting"""
    exp, cnt = GB._expected(oracle, oref, "se", kw, reads, 0)
    got, c15 = {}, {}
    for same_d in settings:
        if same_d is None:
            monkeypatch.delenv("BSX_SAME_D", raising=False)
        else:
            monkeypatch.setenv("BSX_SAME_D", same_d)
        for counters in (False, True):
            bt = B.SingleAlign(gref, len(reads), debug=True)   # (the switch is read when the batch is created)
            try:
                bt.set_work_counters(counters)
                bt.ImportBatchReads([r["seq"] for r in reads], [r["qual"] for r in reads]).Do_Batch()
                res = bt.results()
                GB._compare("se", kw, reads, exp, bt, res, "%s, BSX_SAME_D %s, counters %s" % (route, same_d, counters))
                c = bt.counters()
                print("%s BSX_SAME_D=%s counters=%s: heavy units %d, counter 15 %d, counters 0-3 %s oracle %s" % (route, same_d, counters, bt.heavy_units(), int(c[15]), [int(x) for x in c[:4]], cnt))
                assert bt.heavy_units() > 0
                if same_d == "0" and not grouped_without:
                    assert int(c[15]) == 0, int(c[15])          # no two tasks of equal window and offset
                elif merges:
                    assert int(c[15]) > 0                        # groups of two reads and more: the path ran
                if counters:
                    assert [int(x) for x in c[:4]] == cnt, ([int(x) for x in c[:4]], cnt)
                got[(same_d, counters)] = tuple(a.tobytes() for a in res)
                assert c15.setdefault(same_d, int(c[15])) == int(c[15])   # (the same groups with the work counters off and on)
            finally:
                bt.close()
    assert len(set(got.values())) == 1, [k for k in got if got[k] != got[("0", False)]]
    return exp, c15


def _first_lists(oracle, oref, unit, reads, v):
    al = oracle.OracleAligner(oref, leak_mode=0)
    fh = [(r["L"],) + first_heavy_list(r, unit, GB._exp_read(al.se(i, r["seq"], r["qual"]), al.se_hits, v + 1)["plan"]) for i, r in enumerate(reads)]
    al.free()
    return fh


def _refs(oracle, world, kw):
    oref = oracle.OracleRef(oracle.make_params(**kw), fasta_text=world["fasta"])
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_text=world["fasta"]).CreateIndex()
    return oref, gref


@pytest.mark.parametrize("v", [0, 2, 6])
def test_reads_whose_offsets_differ_by_32(v, world, oracle, monkeypatch):
    kw = dict(s=16, v=v, I=4, S=1, r=1, n=0, f=5)
    oref, gref = _refs(oracle, world, kw)
    try:
        WO.check_buckets(oref, world["pos"])
        B.lib().bsx_set_heavy_threshold(48)
        try:
            for kind, reads, merges in make_batches(world["unit"], v, True):
                if merges:   # the construction holds under the oracle's planner: two five-word reads meet in one window with offsets 32 apart, in the first pass
                    fh = _first_lists(oracle, oref, world["unit"], reads, v)
                    assert any(x[1] == y[1] and y[2] - x[2] == 32 for x in fh for y in fh), fh
                exp, _ = _run(gref, oracle, oref, kw, reads, monkeypatch, "-v %d %s" % (v, kind), merges=merges)
                for r, e in zip(reads, exp):
                    assert not e["filtered"], r["name"]
                    if kind == "over" and r["a"] == 0 and r["L"] == 144:
                        assert e["pick"][0] == 0, (r["name"], e["pick"])                          # one difference too many
                    if kind in ("pristine", "within") and r["a"] == 0 and r["L"] == 144:
                        assert e["pick"][:2] == (len(WO.PRISTINE), 0 if kind == "pristine" else v), (r["name"], e["pick"])   # the unit's own copies
            # the four-word reads on their own: they meet as the five-word ones do, and stay in groups of one — counter 15 is 0 under the default as well
            for kind, reads, merges in make_batches(world["unit"], v, False):
                if merges:
                    fh = _first_lists(oracle, oref, world["unit"], reads, v)
                    assert any(x[1] == y[1] and y[2] - x[2] == 32 for x in fh for y in fh), fh
                _, c15 = _run(gref, oracle, oref, kw, reads, monkeypatch, "-v %d %s, four words" % (v, kind), merges=False)
                assert c15[None] == 0, c15
        finally:
            B.lib().bsx_set_heavy_threshold(0)
    finally:
        gref.close()
        oref.free()


def test_more_congruent_tasks_than_a_group_holds(world, oracle, monkeypatch):
    kw = dict(s=16, v=2, I=4, S=1, r=1, n=0, f=5)
    unit, L = world["unit"], 144
    reads = []
    for a, n in ((0, 20), (32, 6)):
        cs = WO._at(unit[a:a + L], 48, L, "C")   # (anywhere: the index keys do not tell C from T)
        assert len(cs) >= n - 1
        reads += [_read(unit, L, a, 0 if a else 2, 0 if a else 2, drop=cs[i - 1:i] if i else (), tag="twin%d" % i) for i in range(n)]
    assert len({r["seq"] for r in reads}) == len(reads)
    oref, gref = _refs(oracle, world, kw)
    try:
        fh = _first_lists(oracle, oref, unit, reads, 2)
        assert fh == [(144, 32, -32)] * 20 + [(144, 32, 0)] * 6, fh
        B.lib().bsx_set_heavy_threshold(48)
        try:
            exp, _ = _run(gref, oracle, oref, kw, reads, monkeypatch, "twins", merges=True, grouped_without=True)
            for r, e in zip(reads, exp):
                assert e["pick"][0] >= len(WO.PRISTINE) and e["pick"][1] == (0 if r["a"] else 2), (r["name"], e["pick"])
        finally:
            B.lib().bsx_set_heavy_threshold(0)
    finally:
        gref.close()
        oref.free()


def test_three_offset_classes_in_one_window(world, oracle, monkeypatch):
    """L = 132 (five words; one planner start only), -v 6: a = 0, 32 and 64 with four, two and no seeds spoiled meet at unit letter 64 with offsets -64, -32
    and 0, and a = 16 (three spoiled) walks the same window with offset -48.  The default takes the three as one group — the frame moves twice, the whole
    longer gather is used; BSX_SAME_D=1 splits the set behind d = 1 (two reads in a group, the third alone); BSX_SAME_D=0 leaves every read alone.  Counter 15
    counts a window's candidates once per read in a group of two and more, so it grows from setting to setting"""
    v, L, unit = 6, 132, world["unit"]
    kw = dict(s=16, v=v, I=4, S=1, r=1, n=0, f=5)
    oref, gref = _refs(oracle, world, kw)
    try:
        B.lib().bsx_set_heavy_threshold(48)
        try:
            for kind, n, n_at in (("within", v, ()), ("over", v + 1, ()), ("N", v, (L - 2,))):
                reads = [_read(unit, L, a, n, (64 - a) // 16, n_at=n_at, tag=kind) for a in (0, 32, 64, 16)]
                fh = _first_lists(oracle, oref, unit, reads, v)
                assert fh == [(L, 64, -64), (L, 64, -32), (L, 64, 0), (L, 64, -48)], fh
                exp, c15 = _run(gref, oracle, oref, kw, reads, monkeypatch, "three classes, %s" % kind, merges=True, settings=("0", "1", None))
                assert c15["0"] == 0 < c15["1"] < c15[None], c15   # (in the first pass three reads in a group against two; later lists only add to either)
                for r, e in zip(reads, exp):
                    assert (e["pick"][0] == 0) if kind == "over" else (e["pick"][0] >= len(WO.PRISTINE) and e["pick"][1] == v), (r["name"], e["pick"])
        finally:
            B.lib().bsx_set_heavy_threshold(0)
    finally:
        gref.close()
        oref.free()
