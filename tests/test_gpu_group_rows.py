"""k_hscan_same's read loop for the groups of 129-160 nt reads with the work counters off (hs_eval_lean): what only a survivor needs is formed where a
chunk holds one — the task's lane and output address, its survivor count, the list ordinal, the position as the frame's plus 32 d —, the exits of the step's four
chunks are taken together (one test per word on the smallest of a lane's four counts where every lane holds a candidate, four ballots in a window's last step), and
the row may lie in LDS in the order of evaluation and be read in two halves.  Needs an MI355X.

The genome and what its copies are is that of tests/test_gpu_scan_word_order.py: 421 = 256 + 165 copies of one 200-letter unit, every seed of a read made from the
unit one bucket of the copies in position order, heavy threshold 48 — one full step whose four chunks are left behind different words, then a partial step.  The
reads, and the way they are made to meet in one window in the first pass, are those of tests/test_gpu_group_cap.py (make_batch) and tests/test_gpu_offset_classes.py
(_read, first_heavy_list): unit[a : a + L] with its C kept, one difference in every seed before the shared one, told apart by one or two C not kept.  Every batch runs
with the work counters off (the new loop) and on (hs_eval_read, every word in natural order, the rows as they were), under the build's group cap and under
BSX_SAME_R=16 (other cuts: other rows are last, other members are neighbours).  HG_LEAN, HG_SPLIT, HG_JOINT and HG_JOINT_FIRST are build options (a test in the read
loop would cost what they save), so the test runs the forms that the shipped library offers: the default build's (HG_JOINT=3, HG_SPLIT=0), and the unchanged loop
through the counted route; the other positions of the switches ran this file as libraries of their own (BSX_LIB) when they were measured.
Records are compared with the oracle's unit by unit as tests/test_gpu_boundaries.py does, counters 0-3 with the oracle's when counted, and the result bytes of all
routes with each other.

  group sizes: 1, 2, 63, 64 and 65 reads of one window and offset (L = 144, -v 2), every one a hit at the unit's own copies: a task alone (hp_task), the smallest
          group, an odd group whose last row is requested by itself, every lane and every row of UW in use (the last member must not request row 64), and 65 cut
          into 33 + 32.  The member in the last row has survivors, as every member has;
  plain and N alternating: 24 members (L = 144; 18 at L = 129) in turn plain, with an N in word 0, plain, with an N in word 4 (144 only: the 129th letter is
          all of word 4), plain, with an N in word 2 — a half requested ahead then belongs to a read of the other form than the one being evaluated;
  words needed in one chunk only: worlds of their own, built by the same builder with its constants patched (every copy but the unit's own differs from the unit in
          word 0, so every chunk without the unit is left behind the first evaluated word): the unit at lanes 0 and 63 of chunk 1 only — chunk 1 takes every
          word, the other three chunks of its step and the whole partial step none but the first; the unit only in the last lane of the partial last chunk, 421
          copies (chunk u = 2 of the second step, lane 36) and 460 copies (u = 3, lane 11): the exit of a step whose lanes do not all hold a candidate must OR
          all four chunks.  Groups of 144- and 129-letter reads; what each chunk does to a member is asserted letter by letter first (chunk_profile), as it is
          for the shared world (test_what_the_chunks_of_the_world_do_to_a_member: there chunks 2 and 3 are left behind the LAST word without a survivor);
  survivors of different counts: a world whose copies carry ONE difference from the unit (word 2) and that holds the unit at entries 100, 230 and 300: to a pristine
          read the first hundred entries are hits of class 1, entry 100 — lane 36 of the first step's second chunk — is a hit of class 0, and the threshold falls
          inside the list: the survivors recorded behind it are replayed under the new threshold, each with its whole count;
  offset classes: three classes d = 0, 1, 2 of 6 reads each (L = 132, -v 6) and two of 5 (L = 144, -v 2), every read a hit: the position a survivor reports is
          the frame's plus 32 d, formed where it is written;
  overflow: a second world of 700 copies of which 540 are the unit itself (the same construction, the constants of test_gpu_scan_word_order patched while it is
          built): a member that is a hit at all of them has more survivors than a task's list holds (512) and is done again by the control kernel, beside
          neighbours with one difference too many, which have none;
  lengths and thresholds: groups of 9 reads of 144 and of 129 letters, -v 0, 2 and 6, plain, with members over the threshold and with members that carry an N."""
import contextlib
import itertools

import pytest

import bsmap_amd as B
import bsx_testdata as td
import test_gpu_boundaries as GB
import test_gpu_group_cap as GC
import test_gpu_offset_classes as OC
import test_gpu_scan_word_order as WO

pytestmark = pytest.mark.gpu

KW = {v: dict(s=16, v=v, I=4, S=1, r=1, n=0, f=5) for v in (0, 2, 6)}
EVAL_ORDER = (0, 4, 3, 2, 1)


@pytest.fixture(scope="module")
def world(oracle):
    """the genome, and per -v the reference on both sides (made once: the tests only read them), with the heavy threshold at 48 while the module runs"""
    g, unit, copies, pos = WO.make_genome()
    w = dict(fasta=td.fasta_text(g), unit=unit, copies=copies, pos=pos, refs={})
    for v, kw in KW.items():
        oref = oracle.OracleRef(oracle.make_params(**kw), fasta_text=w["fasta"])
        gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_text=w["fasta"]).CreateIndex()
        w["refs"][v] = (oref, gref)
    WO.check_buckets(w["refs"][2][0], pos)
    B.lib().bsx_set_heavy_threshold(48)
    try:
        yield w
    finally:
        B.lib().bsx_set_heavy_threshold(0)
        for oref, gref in w["refs"].values():
            gref.close()
            oref.free()


def chunk_profile(seq, copies, thr):
    """per chunk of 64 copies: (words evaluated in the order 0, 4, 3, 2, 1 with a test behind every word, lanes within the threshold behind the last)"""
    out = []
    for c0 in range(0, len(copies), 64):
        tot = [0] * len(copies[c0:c0 + 64])
        words = 0
        for j in EVAL_ORDER:
            a, b = 32 * j, min(32 * j + 32, len(seq))
            tot = [t + WO._counted(seq[a:b], cp[a:b]) for t, cp in zip(tot, copies[c0:c0 + 64])]
            words += 1
            if not any(t <= thr for t in tot):
                break
        out.append((words, [l for l, t in enumerate(tot) if t <= thr] if words == 5 else []))
    return out


def first_lists(world, oracle, reads, v):
    return [x[1:] for x in OC._first_lists(oracle, world["refs"][v][0], world["unit"], reads, v)]


def run(refs, oracle, kw, reads, monkeypatch, route, grouped=True):
    """one batch through BSX_SAME_R unset and =16 and both settings of the work counters, against the oracle"""
    oref, gref = refs
    exp, cnt = GB._expected(oracle, oref, "se", kw, reads, 0)
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
                assert bt.heavy_units() > 0
                assert (int(c[15]) > 0) == grouped, int(c[15])   # hs_group ran: candidates evaluated in groups of two reads and more
                if counters:
                    assert [int(x) for x in c[:4]] == cnt, ([int(x) for x in c[:4]], cnt)
                got[(same_r, counters)] = tuple(a.tobytes() for a in res)
            finally:
                bt.close()
    assert len(set(got.values())) == 1, [k for k in got if got[k] != got[(None, False)]]
    return exp


def one_window(world, oracle, reads, v, meet):
    """every read's first heavy list is the window at unit letter `meet`, at its own offset (checked against the oracle's plan before anything is asked of the device)"""
    fh = first_lists(world, oracle, reads, v)
    if meet is None:   # (-v 0: one seed, where the planner starts in the read's first letters — the same for every read of one length and offset)
        assert fh[0][0] is not None and fh == [fh[0]] * len(reads), fh
    else:
        assert fh == [(meet, r["a"] - meet) for r in reads], fh


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_group_sizes(n, world, oracle, monkeypatch):
    reads = GC.make_batch(world["unit"], 144, 2, (n,), "plain")
    one_window(world, oracle, reads, 2, 32)
    exp = run(world["refs"][2], oracle, KW[2], reads, monkeypatch, "group of %d" % n, grouped=n > 1)
    for r, e in zip(reads, exp):   # every member, the one in the last row among them, has survivors: the unit's own copies
        assert not e["filtered"] and e["pick"][0] >= len(WO.PRISTINE) and e["pick"][1] == 2, (r["name"], e["pick"])


def alternating(unit, L, v, n):
    """n reads of unit[:L], in turn plain and with an N in word 0, word 4 (where the read has more than one letter there) and word 2"""
    spoil = 2 if v else 0
    n_words = [None, 0, None, 4, None, 2] if L > 129 else [None, 0, None, 2]
    at = {0: 30, 4: L - 2, 2: 70}
    out = []
    for i, drop in zip(range(n), GC._drops(unit, L, 0)):
        w = n_words[i % len(n_words)]
        out.append(OC._read(unit, L, 0, v, spoil, n_at=() if w is None else (at[w],), drop=tuple(d for d in drop if w is None or d != at[w]), tag="%s%d" % ("plain" if w is None else "N%d_" % w, i)))
    assert len({r["seq"] for r in out}) == n
    return out


@pytest.mark.parametrize("L,n", [(144, 24), (129, 18)])
def test_plain_and_N_reads_alternate(L, n, world, oracle, monkeypatch):
    reads = alternating(world["unit"], L, 2, n)
    one_window(world, oracle, reads, 2, 32)
    exp = run(world["refs"][2], oracle, KW[2], reads, monkeypatch, "alternating, %d letters" % L)
    for r, e in zip(reads, exp):
        assert not e["filtered"] and e["pick"][0] >= len(WO.PRISTINE) and e["pick"][1] == 2, (r["name"], e["pick"])


def test_what_the_chunks_of_the_world_do_to_a_member(world):
    """the claims of the module text about the chunks, letter by letter (no device: they are what makes the other cases reach every arm of the loop)"""
    for L, v in ((144, 2), (129, 2), (144, 6), (132, 6)):
        r = GC.make_batch(world["unit"], L, v, (1,), "plain")[0]
        p = chunk_profile(r["seq"], [c[:L] for c in world["copies"]], v)
        assert [x[0] for x in p] == [1, 5, 5, 5, 5, 4, 5], (L, v, p)   # chunk 0 behind the first word, chunk 5 behind word 2; the others through all five
        assert [x[1] for x in p] == [[], [0, 63], [], [], [0], [], [36]], (L, v, p)   # survivors: the unit's copies only — chunk 1's both ends, the partial chunk's last lane
    assert len(world["copies"]) - 6 * 64 == 37


@pytest.mark.parametrize("L,v,sizes,meet", [(132, 6, (6, 6, 6), 64), (144, 2, (5, 5), 32)])
def test_survivors_in_every_offset_class(L, v, sizes, meet, world, oracle, monkeypatch):
    reads = GC.make_batch(world["unit"], L, v, sizes, "plain")
    one_window(world, oracle, reads, v, meet)
    exp = run(world["refs"][v], oracle, KW[v], reads, monkeypatch, "classes of %s" % (sizes,))
    for r, e in zip(reads, exp):   # (the positions are compared with the oracle's in run: a class's are the frame's plus 32 d)
        assert not e["filtered"] and e["pick"][0] >= len(WO.PRISTINE), (r["name"], e["pick"])
    assert {r["a"] for r in reads} == {32 * d for d in range(len(sizes))}


def uniform(unit, L, v, n, kind):
    """n reads of unit[:L] that walk one window with one offset; kind as in test_gpu_group_cap.make_batch ('over' and 'N' members at reads 0, 4 and 8)"""
    if v:
        spoil, meet = 2, 32
    else:
        spoil, meet = 0, None   # (-v 0: one seed, in the read's first letters)
    out = []
    for i, drop in zip(range(n), GC._drops(unit, L, 0)):
        sp = i % 4 == 0
        if sp and kind == "over":
            out.append(OC._read(unit, L, 0, v + 1, spoil, drop=drop, tag="over%d" % i))
        elif sp and kind == "N":
            out.append(OC._read(unit, L, 0, v, spoil, n_at=(L - 2,) if L > 129 else (70,), drop=tuple(d for d in drop if d != 70), tag="N%d" % i))
        else:
            out.append(OC._read(unit, L, 0, v, spoil, drop=drop, tag="twin%d" % i))
    assert len({r["seq"] for r in out}) == n
    return out, meet


@pytest.mark.parametrize("kind", ["plain", "over", "N"])
@pytest.mark.parametrize("v", [0, 2, 6])
@pytest.mark.parametrize("L", [144, 129])
def test_lengths_and_thresholds(L, v, kind, world, oracle, monkeypatch):
    reads, meet = uniform(world["unit"], L, v, 9, kind)
    one_window(world, oracle, reads, v, meet)
    exp = run(world["refs"][v], oracle, KW[v], reads, monkeypatch, "%d letters, -v %d, %s" % (L, v, kind))
    for r, e in zip(reads, exp):
        assert not e["filtered"], r["name"]
        if "_over" in r["name"]:
            assert e["pick"][0] == 0, (r["name"], e["pick"])
        else:
            assert e["pick"][0] >= len(WO.PRISTINE) and e["pick"][1] == v, (r["name"], e["pick"])


@contextlib.contextmanager
def patched_world(oracle, monkeypatch, n_copies, pristine, sets, v=2, cluster=None):
    """a world of test_gpu_scan_word_order's builder with other constants: n_copies copies, the unit itself at `pristine`, every other copy of every chunk with
    the difference sets `sets` (and `cluster` differences per word instead of 7); heavy threshold 48 while it is in use"""
    with monkeypatch.context() as m:
        m.setattr(WO, "N_COPIES", n_copies)
        m.setattr(WO, "PRISTINE", tuple(pristine))
        m.setattr(WO, "CHUNK_SETS", {c: sets for c in range((n_copies + 63) // 64)})
        if cluster is not None:
            m.setattr(WO, "CLUSTER", cluster)
        g, unit, copies, pos = WO.make_genome()
    assert len(copies) == n_copies and [c for c, t in enumerate(copies) if t == unit] == list(pristine)
    fasta = td.fasta_text(g)
    oref = oracle.OracleRef(oracle.make_params(**KW[v]), fasta_text=fasta)
    gref = B.RefSeq(B.make_params(**KW[v])).Run_ConvertBinseq(fasta_text=fasta).CreateIndex()
    B.lib().bsx_set_heavy_threshold(48)
    try:
        yield dict(unit=unit, copies=copies, pos=pos, refs={v: (oref, gref)})
    finally:
        B.lib().bsx_set_heavy_threshold(0)
        gref.close()
        oref.free()


def same_window(w, oracle, reads, v):
    """the reads of one length and offset walk one window with one offset as their first heavy list (the oracle's plan)"""
    fh = first_lists(w, oracle, reads, v)
    for key in {(r["L"], r["a"]) for r in reads}:
        mine = [x for x, r in zip(fh, reads) if (r["L"], r["a"]) == key]
        assert mine[0][0] is not None and mine == [mine[0]] * len(mine), (key, fh)


@pytest.mark.parametrize("n_copies,pristine,words,survivors", [
    (421, (64, 127), [1, 5, 1, 1, 1, 1, 1], {1: [0, 63]}),        # chunk 1 alone needs every word: the unit at its lanes 0 and 63
    (421, (420,), [1, 1, 1, 1, 1, 1, 5], {6: [36]}),              # the partial last chunk's last lane: chunk u = 2 of the second step
    (460, (459,), [1, 1, 1, 1, 1, 1, 1, 5], {7: [11]}),           # the same in chunk u = 3 of the second step
])
def test_words_needed_in_one_chunk_only(n_copies, pristine, words, survivors, oracle, monkeypatch):
    with patched_world(oracle, monkeypatch, n_copies, pristine, ((0,),)) as w:
        reads = GC.make_batch(w["unit"], 144, 2, (5,), "plain") + GC.make_batch(w["unit"], 129, 2, (4,), "plain")
        for r in reads:   # what the case claims, letter by letter
            p = chunk_profile(r["seq"], [c[:r["L"]] for c in w["copies"]], 2)
            assert [x[0] for x in p] == words and [x[1] for x in p] == [survivors.get(c, []) for c in range(len(p))], (r["name"], p)
        same_window(w, oracle, reads, 2)
        exp = run(w["refs"][2], oracle, KW[2], reads, monkeypatch, "the unit at %s of %d" % (pristine, n_copies))
        for r, e in zip(reads, exp):
            assert not e["filtered"] and e["pick"][:2] == (len(pristine), 2), (r["name"], e["pick"])


def test_a_hit_lowers_the_threshold_inside_a_list(oracle, monkeypatch):
    """entries 0-99 are hits of class 1, entry 100 (second chunk, lane 36) of class 0: 421 survivors of two counts in one list, replayed under a threshold that falls"""
    with patched_world(oracle, monkeypatch, 421, (100, 230, 300), ((2,),), cluster=1) as w:
        reads = GC._class(w["unit"], 144, 32, 4, 2, (), "plain")   # unit[32 : 176], no difference: their first heavy list is their first seed
        for r in reads:
            d = [WO._counted(r["seq"], t[32:176]) for t in w["copies"]]
            assert [c for c, x in enumerate(d) if x == 0] == [100, 230, 300] and set(d) == {0, 1}, r["name"]
        same_window(w, oracle, reads, 2)
        exp = run(w["refs"][2], oracle, KW[2], reads, monkeypatch, "survivors of two counts")
        for r, e in zip(reads, exp):
            assert not e["filtered"] and e["pick"][:2] == (3, 0), (r["name"], e["pick"])


def test_one_member_overflows_its_survivor_list(oracle, monkeypatch):
    """700 copies, 540 of them the unit itself: a hit at all of them is more than the 512 survivors a task's list holds.  The 512th of them is copy 611, lane 35 of the
    third step's second chunk.  With the work counters off the control kernel replays the 512 recorded survivors and walks the list on from the last one's ordinal + 1:
    an ordinal that is too large loses the unit's copies behind it (a build with the ordinal 64 too large fails here), one that is too small only walks candidates again
    whose hits the unit's hit set already holds (a build whose ordinal lacks its chunk passes: more work, the same records)"""
    n_copies, pristine = 700, tuple(range(100, 640))
    assert (pristine[511] // 64) % 4 == 1
    with monkeypatch.context() as m:
        m.setattr(WO, "N_COPIES", n_copies)
        m.setattr(WO, "PRISTINE", pristine)
        m.setattr(WO, "CHUNK_SETS", {c: ((0,),) for c in range((n_copies + 63) // 64)})
        g, unit, copies, pos = WO.make_genome(seed=78)
    assert len(copies) == n_copies and sum(1 for c in copies if c == unit) == len(pristine) > 512
    fasta = td.fasta_text(g)
    kw = KW[2]
    oref = oracle.OracleRef(oracle.make_params(**kw), fasta_text=fasta)
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_text=fasta).CreateIndex()
    try:
        # members 0 and 2 carry one difference too many (no survivor), member 1 is a hit at every copy that is the unit: the one that overflows between two that do not
        drops = list(itertools.islice(GC._drops(unit, 144, 0), 5))
        reads = [OC._read(unit, 144, 0, 3 if i != 1 else 2, 2, drop=drops[i], tag="%s%d" % ("over" if i != 1 else "all", i)) for i in range(5)]
        fh = [x[1:] for x in OC._first_lists(oracle, oref, unit, reads, 2)]
        assert fh[0][0] is not None and fh == [fh[0]] * 5, fh   # one window, one offset
        B.lib().bsx_set_heavy_threshold(48)
        try:
            exp = run((oref, gref), oracle, kw, reads, monkeypatch, "overflow")
        finally:
            B.lib().bsx_set_heavy_threshold(0)
        for r, e in zip(reads, exp):
            assert not e["filtered"], r["name"]
            assert e["pick"][0] == (0 if "_over" in r["name"] else len(pristine)), (r["name"], e["pick"])
    finally:
        gref.close()
        oref.free()
