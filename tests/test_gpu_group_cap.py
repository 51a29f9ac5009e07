"""k_hscan_same's groups of up to 64 reads (HG_R, BSX_SAME_R): every read that walks one window with one offset — or with offsets 32 d apart — in one 64-slot
segment of the scan order shares one fetch and one shift of the candidates' reference, a row of LDS and a lane of the wave each.  Needs an MI355X.

The genome and what its copies are is that of tests/test_gpu_scan_word_order.py (421 copies of one 200-letter unit, every seed of a read made from the unit one
bucket of the copies, heavy threshold 48), the reads and the way they are made to meet in one window in the first pass are those of
tests/test_gpu_offset_classes.py: unit[a : a + L] with its C kept, one difference in every seed before the shared one.  The reads of one (L, a) here differ in
one or two C not kept (T under the genome's C is not counted), so every one is a distinct read, a task of its own, and a hit wherever its class has one.

Every batch runs under four routes — BSX_SAME_R unset (the build's cap) and =16 (round 8's groups and task order), each with the work counters off and on.
Records are compared with the oracle's unit by unit as tests/test_gpu_boundaries.py does, counters 0-3 with the oracle's when counted, and the result bytes
of the four routes with each other.  Counter 15 (candidates evaluated in groups of two reads and more) must be above 0 on every route.
  one class: L = 144, a = 0, -v 2, n = 17, 33, 48, 49, 64, 65, 80 reads: the caps of every build and one more, a group that fills every lane (64), sets that
          cross the 64-slot segment of k_task_groups (65, 80); 17 under BSX_SAME_R=16 is a full group and a group of one;
  two classes: L = 144, a = 0 and 32, 40 + 30 and 60 + 10: the cap of 64 falls inside the second class, that of 16 inside the first;
  three classes: L = 132, -v 6, a = 0, 32 and 64 (as the third test of test_gpu_offset_classes builds them), 30 + 30 + 30;
  four words: L = 100, a = 0, 40 reads of one offset (the form that keeps every word: the cap is the same for every length class);
each of them plain, once with members that carry v + 1 differences (no hit, every list walked: a row that yields no survivor) and once with members that carry
an N in the last word (the evaluation with three operations per word).  Those members stand at the first read of every class and at reads 15, 16, 63 and 64 of the
batch, counted over its classes in order — the rows on both sides of either cap's cut, since a group's rows are sorted by class: in 40 + 30 the cut of 64 lies between
reads 23 and 24 of the second class, in 60 + 10 between its reads 3 and 4, in 30 + 30 + 30 between reads 3 and 4 of the third (the second ballot of k_task_groups with
members already taken, and hs_group's frame moved down before the group's last row).  A row's place in its group follows the order in which the tasks arrive in their
bin, which for one block of tasks is nearly the reads' order but is not promised: what is asked is that every read of the batch, such a member and each of its
neighbours, is the oracle's record wherever the member's row lies.

That the large groups formed is read from the kernel's own statistics: 40 same-offset reads with BSX_SIGHIST=1 print a `[sighist] scan kernel` line whose mean
group is above 16 under the default cap and at most 16 under BSX_SAME_R=16."""
import itertools
import re

import pytest

import bsmap_amd as B
import bsx_testdata as td
import test_gpu_boundaries as GB
import test_gpu_offset_classes as OC
import test_gpu_scan_word_order as WO

pytestmark = pytest.mark.gpu

KW2 = dict(s=16, v=2, I=4, S=1, r=1, n=0, f=5)
KW6 = dict(s=16, v=6, I=4, S=1, r=1, n=0, f=5)


@pytest.fixture(scope="module")
def world(oracle):
    """the genome, and per -v the reference on both sides (made once: the tests only read them), with the heavy threshold at 48 while the module runs"""
    g, unit, copies, pos = WO.make_genome()
    w = dict(fasta=td.fasta_text(g), unit=unit, copies=copies, pos=pos, refs={})
    for kw in (KW2, KW6):
        oref = oracle.OracleRef(oracle.make_params(**kw), fasta_text=w["fasta"])
        gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_text=w["fasta"]).CreateIndex()
        w["refs"][kw["v"]] = (oref, gref)
    WO.check_buckets(w["refs"][2][0], pos)
    B.lib().bsx_set_heavy_threshold(48)
    try:
        yield w
    finally:
        B.lib().bsx_set_heavy_threshold(0)
        for oref, gref in w["refs"].values():
            gref.close()
            oref.free()


def _drops(unit, L, a):
    """sets of C not kept that tell the reads of one (L, a) apart: none, every one, every two (anywhere behind letter 48: the index keys do not tell C from T)"""
    cs = WO._at(unit[a:a + L], 48, L - 2, "C")
    return itertools.chain([()], ((c,) for c in cs), itertools.combinations(cs, 2))


def _class(unit, L, a, n, v, special, kind):
    """n distinct reads of unit[a : a + L] that meet the other classes' at unit letter `meet`: v differences (none where no seed has to be spoiled and the class is the
    window's own), one in each seed before the shared one; the reads at the indices of `special` carry v + 1 differences (kind 'over') or an N in the last word ('N')"""
    meet = 64 if L == 132 else 32
    spoil = (meet - a) // 16
    base = v if spoil else 0
    out = []
    for i, drop in zip(range(n), _drops(unit, L, a)):
        if i in special and kind == "over":
            out.append(OC._read(unit, L, a, v + 1, spoil, drop=drop, tag="over%d" % i))
        elif i in special and kind == "N":
            out.append(OC._read(unit, L, a, v, spoil, n_at=(L - 2,), drop=drop, tag="N%d" % i))
        else:
            out.append(OC._read(unit, L, a, base, spoil, drop=drop, tag="twin%d" % i))
    assert len(out) == n
    return out


def make_batch(unit, L, v, sizes, kind):
    """the classes a = 0, 32, ... of the given sizes in one batch; kind: 'plain', 'over' or 'N' (see the module text for where those members stand)"""
    reads = []
    for c, n in enumerate(sizes):
        before = sum(sizes[:c])
        # read 0 of every class; the reads on both sides of either cap's cut: reads 15 | 16 and 63 | 64 of the batch, whichever class they fall into
        special = () if kind == "plain" else tuple(sorted({0} | {i - before for i in (15, 16, 63, 64) if 0 <= i - before < n}))
        reads += _class(unit, L, 32 * c, n, v, special, kind)
    assert len({r["seq"] for r in reads}) == len(reads)
    return reads


def _run(world, oracle, kw, reads, monkeypatch, route, meet):
    """one batch through BSX_SAME_R unset and =16 and both settings of the work counters, against the oracle.  meet: the unit letter of the window in which every
    read's first heavy list lies (checked against the oracle's plan before anything is asked of the device)"""
    oref, gref = world["refs"][kw["v"]]
    exp, cnt = GB._expected(oracle, oref, "se", kw, reads, 0)
    fh = [OC.first_heavy_list(r, world["unit"], e["plan"]) for r, e in zip(reads, exp)]
    assert fh == [(meet, r["a"] - meet) for r in reads], fh
    got = {}
    for same_r in (None, "16"):
        if same_r is None:
            monkeypatch.delenv("BSX_SAME_R", raising=False)
        else:
            monkeypatch.setenv("BSX_SAME_R", same_r)
        for counters in (False, True):
            bt = B.SingleAlign(gref, len(reads), debug=True)   # (the switch is read when the batch is created)
            try:
                bt.set_work_counters(counters)
                bt.ImportBatchReads([r["seq"] for r in reads], [r["qual"] for r in reads]).Do_Batch()
                res = bt.results()
                GB._compare("se", kw, reads, exp, bt, res, "%s, BSX_SAME_R %s, counters %s" % (route, same_r, counters))
                c = bt.counters()
                print("%s BSX_SAME_R=%s counters=%s: heavy units %d, counter 15 %d, counters 0-3 %s oracle %s" % (route, same_r, counters, bt.heavy_units(), int(c[15]), [int(x) for x in c[:4]], cnt))
                assert bt.heavy_units() > 0 and int(c[15]) > 0, (bt.heavy_units(), int(c[15]))   # hs_group ran
                if counters:
                    assert [int(x) for x in c[:4]] == cnt, ([int(x) for x in c[:4]], cnt)
                got[(same_r, counters)] = tuple(a.tobytes() for a in res)
            finally:
                bt.close()
    assert len(set(got.values())) == 1, [k for k in got if got[k] != got[(None, False)]]
    return exp


def _check_picks(reads, exp):
    for r, e in zip(reads, exp):
        assert not e["filtered"], r["name"]
        if "_over" in r["name"]:
            assert e["pick"][0] == 0, (r["name"], e["pick"])                       # one difference too many
        else:
            assert e["pick"][0] >= len(WO.PRISTINE), (r["name"], e["pick"])        # the unit's own copies at least


@pytest.mark.parametrize("kind", ["plain", "over", "N"])
@pytest.mark.parametrize("n", [17, 33, 48, 49, 64, 65, 80])
def test_one_class(n, kind, world, oracle, monkeypatch):
    reads = make_batch(world["unit"], 144, 2, (n,), kind)
    exp = _run(world, oracle, KW2, reads, monkeypatch, "one class of %d, %s" % (n, kind), 32)
    _check_picks(reads, exp)


@pytest.mark.parametrize("kind", ["plain", "over", "N"])
@pytest.mark.parametrize("sizes", [(40, 30), (60, 10)])
def test_two_classes_in_one_window(sizes, kind, world, oracle, monkeypatch):
    reads = make_batch(world["unit"], 144, 2, sizes, kind)
    exp = _run(world, oracle, KW2, reads, monkeypatch, "classes of %s, %s" % (sizes, kind), 32)
    _check_picks(reads, exp)


@pytest.mark.parametrize("kind", ["plain", "over", "N"])
def test_three_classes_in_one_window(kind, world, oracle, monkeypatch):
    reads = make_batch(world["unit"], 132, 6, (30, 30, 30), kind)
    exp = _run(world, oracle, KW6, reads, monkeypatch, "three classes of 30, %s" % kind, 64)
    _check_picks(reads, exp)


@pytest.mark.parametrize("kind", ["plain", "over", "N"])
def test_four_words(kind, world, oracle, monkeypatch):
    reads = make_batch(world["unit"], 100, 2, (40,), kind)
    exp = _run(world, oracle, KW2, reads, monkeypatch, "four words, 40 reads, %s" % kind, 32)
    _check_picks(reads, exp)


def _mean_group(world, reads, capfd):
    gref = world["refs"][2][1]
    bt = B.SingleAlign(gref, len(reads), debug=True)
    try:
        bt.ImportBatchReads([r["seq"] for r in reads], [r["qual"] for r in reads]).Do_Batch()
        capfd.readouterr()
        c = bt.counters()
    finally:
        bt.close()
    err = capfd.readouterr().err
    m = re.findall(r"\[sighist\] scan kernel: ([0-9.]+) of the candidates in groups, mean group ([0-9.]+) reads", err)
    assert m, err
    assert int(c[15]) > 0
    return float(m[-1][1])


def test_the_large_groups_form(world, oracle, monkeypatch, capfd):
    """40 reads of one window and offset: one group of 40 under the build's cap wherever that is above 16, groups of 16, 16 and 8 under BSX_SAME_R=16"""
    reads = make_batch(world["unit"], 144, 2, (40,), "plain")
    monkeypatch.setenv("BSX_SIGHIST", "1")
    monkeypatch.delenv("BSX_SAME_R", raising=False)
    mg = _mean_group(world, reads, capfd)
    monkeypatch.setenv("BSX_SAME_R", "16")
    mg16 = _mean_group(world, reads, capfd)
    print("mean group: default cap %.2f, BSX_SAME_R=16 %.2f" % (mg, mg16))
    assert mg > 16.0, mg
    assert mg16 <= 16.0, mg16
