"""The exiting evaluation of k_hscan_same's WGBS groups (same_exit: a read's words one at a time — 0, 4, 3, 2, 1 for reads of 129-160 nt — and a chunk of 64
candidates left as soon as none of them is within the threshold) on directed reads, against the oracle.  Needs an MI355X.  Reads of 129-160 nt take the exiting
form; the same cases at 128, 100 and 80 letters run the forms that keep every word (four words, any length) on the same genome.

The genome is one chromosome of random sequence with 421 copies of one 200-letter unit, every copy at a position that is a multiple of 4 (-I 4).  A copy
differs from the unit ONLY in letters where the unit has C and the copy T: the index keys (C = T) of all copies are the unit's, so every seed of a read made
from the unit is one bucket of exactly the 421 copies in position order (checked against the oracle's index below) — entry i of every list is copy i,
whichever seeds the planner chooses — and the reads are the unit's letters with their C KEPT (a methylated read), so that a copy's T under a read's C is a
counted difference.  With the heavy threshold at 48 those lists are deferred, and reads that walk the same seed are tasks of equal window and offset:
k_hscan_same takes them as groups (counter 15).  421 = 256 + 165 entries: one full step of four chunks, then a step whose last chunk holds 37 candidates.

The copies, by chunk of 64 entries (a copy carries 7 differences in every word of its set, so it is over every threshold used here inside that word):
  chunk 0: word 0;  chunk 1: the unit itself at entries 0 and 63, the others word 0 or words 4 and 2;  chunk 2: a mix of all sets;  chunk 3: word 1;
  chunk 4: words 3 and 1;  chunk 5 (second step): the unit at entry 0, the others word 2;  chunk 6 (37 entries): a mix, and the unit at the last entry.
So the chunks are left behind different words, the only candidates within the threshold are the four copies of the unit — lanes 0 and 63 of a full chunk,
lane 0 of the second step's first chunk and the last lane of the partial chunk —, and every set reaches into the first 80 letters, so that this holds at
every read length.  Every case is built at 144 and 129 letters (five words, the last of 16 and of 1 letter), 128 and 100 (four words), 80 (any length),
with -v 0, 2 and 6; differences of the READ from the unit are G <-> A changes as bsx_testdata.directed_read places them:
  word k, for every word of the read: exactly v differences, all inside word k — four hits of class v, at the unit's copies — and v + 1: no hit.  Where
         word k of the read holds fewer letters that can carry a difference than the case needs (the 1-letter word of a 129-letter read with v > 0, the
         4-letter word of a 100-letter read with v = 6) the case does not exist and is not built;
  first+last: v differences in word 0, the first evaluated, and one more in the word evaluated last (word 1 of five, else the read's last): no hit;
  N in word j, for every word: one N there (the form with three operations per word) and v, or v + 1, differences in the next word.
Every read has a twin that differs in one letter outside the case's word (one C not kept), so that groups of two and more exist.  What each case claims is
checked in Python first (the counted differences of every read against every copy, letter by letter); then the device's records — work counters off (the
exiting form) and on (every word, natural order) — are compared unit by unit with the oracle as tests/test_gpu_boundaries.py does, and the result bytes
of the two runs with each other."""
import numpy as np
import pytest

import bsmap_amd as B
import bsx_testdata as td
import test_gpu_boundaries as GB

pytestmark = pytest.mark.gpu

UNIT, N_COPIES, CLUSTER = 200, 421, 7
PRISTINE = (64, 127, 256, 420)                          # the copies that are the unit itself
LENGTHS = (144, 129, 128, 100, 80)
LAST_EVALUATED = {144: 1, 129: 1, 128: 3, 100: 3, 80: 2}
WORD = {0: (0, 32), 1: (32, 64), 2: (64, 80), 3: (100, 128), 4: (128, 144)}   # where a copy's differences of a word lie: inside every read length that has the word
SETS = ((0,), (1,), (2,), (3, 1), (4, 2))
CHUNK_SETS = {0: ((0,),), 1: ((0,), (4, 2)), 2: SETS, 3: ((1,),), 4: ((3, 1),), 5: ((2,),), 6: SETS}


def _at(text, a, b, letters):
    return [i for i in range(a, min(b, len(text))) if text[i] in letters]


def _counted(read, ref):
    """differences the 3-letter comparison counts between a read of the forward strand and forward reference letters"""
    return sum(1 for r, g in zip(read, ref) if r != "N" and r != g and not (r == "T" and g == "C"))


def make_genome(seed=77):
    rng = np.random.default_rng(seed)
    mix = lambda n, c, ga: "".join(rng.permutation(list("C" * c + "".join(rng.choice(list("GA"), ga)) + "T" * (n - c - ga))))
    # every word's part of WORD holds 7 C and at least 7 G / A (the letters that carry a copy's and a read's differences); letter 128 and letters 96-99 carry a read's
    unit = mix(32, 9, 14) + mix(32, 9, 14) + mix(16, 7, 8) + mix(16, 4, 8) + "GAGA" + mix(28, 9, 12) + "G" + mix(15, 7, 7) + mix(56, 14, 28)
    assert len(unit) == UNIT
    copies = []
    for c in range(N_COPIES):
        t = list(unit)
        if c not in PRISTINE:
            sets = CHUNK_SETS[c // 64]
            for w in sets[c % len(sets)]:
                for i in rng.choice(_at(unit, *WORD[w], "C"), CLUSTER, replace=False):
                    t[int(i)] = "T"
        copies.append("".join(t))
    parts, pos = [], []
    at = 0
    for t in copies:
        sp = td.random_seq(rng, 4 * int(rng.integers(50, 100)), 0.5).tobytes().decode()
        parts += [sp, t]
        pos.append(at + len(sp))
        at += len(sp) + UNIT
    parts.append(td.random_seq(rng, 400, 0.5).tobytes().decode())
    return [("chrR", "".join(parts))], unit, copies, pos


def make_reads(unit, v):
    """the directed reads of one -v: dicts with the read, the differences placed in it and what it must be: ('hit', class) at the unit's copies, or ('none',)"""
    out = []

    def add(cls, L, k, subs=(), n_at=(), want=None):
        u = unit[:L]
        conv = td.directed_read(u, "++", subs=subs, n_at=n_at)
        keep = [i for i in range(L) if u[i] == "C" and conv[i] != "N"]
        nk = (k + 1) % ((L + 31) // 32) if L > 32 * k + 32 or k else 1
        drop = [i for i in keep if 32 * nk <= i < 32 * nk + 32][:1]   # the twin: one C of another word not kept
        for tw, dr in (("a", []), ("b", drop)):
            seq = "".join("C" if i in keep and i not in dr else conv[i] for i in range(L))
            out.append(dict(name="%s_L%d_%d%s" % (cls, L, len(out), tw), seq=seq, qual="I" * L, cls=cls, L=L, k=k, want=want, subs=tuple(subs)))

    for L in LENGTHS:
        nw = (L + 31) // 32
        u = unit[:L]
        for k in range(nw):
            car = _at(u, 32 * k, 32 * k + 32, "GA")
            for n, want in ((v, ("hit", v)), (v + 1, ("none",))):
                if len(car) >= n:
                    add("word%d" % k, L, k, subs=car[:n], want=want)
                    if n:
                        add("word%d" % k, L, k, subs=car[len(car) - n:], want=want)
        kl = LAST_EVALUATED[L]
        add("firstlast", L, 0, subs=_at(u, 0, 32, "GA")[:v] + _at(u, 32 * kl, 32 * kl + 32, "GA")[-1:], want=("none",))
        for j in range(nw):
            k = (j + 1) % nw
            n_at = (min(32 * j + 28, L - 1),)
            car = [i for i in _at(u, 32 * k, 32 * k + 32, "GA") if i not in n_at]
            for n, want in ((v, ("hit", v)), (v + 1, ("none",))):
                if len(car) >= n:
                    add("N%d" % j, L, k, subs=car[:n], n_at=n_at, want=want)
    return out


def check_claims(reads, unit, copies, v):
    """every read is what its case says, counted letter by letter against every copy"""
    for r in reads:
        L = r["L"]
        d = [_counted(r["seq"], t[:L]) for t in copies]
        diff_at = [i for i in range(L) if _counted(r["seq"][i], unit[i])]
        assert sorted(diff_at) == sorted(r["subs"]), r["name"]                  # the differences from the unit lie where they were placed
        if r["cls"].startswith("word"):
            assert all(32 * r["k"] <= i < 32 * r["k"] + 32 for i in diff_at) and len(diff_at) in (v, v + 1), r["name"]
        near = [c for c, x in enumerate(d) if x <= v]
        if r["want"][0] == "hit":   # the unit's copies, with exactly the placed differences, are the only candidates within the threshold
            assert near == list(PRISTINE) and all(d[c] == r["want"][1] for c in PRISTINE), (r["name"], near)
        else:
            assert near == [] and all(d[c] == v + 1 for c in PRISTINE), (r["name"], near)


def check_buckets(oref, pos):
    """the forward buckets that hold a copy hold all of them, in position order: entry i of a list is copy i (a seed or two may also occur elsewhere by chance)"""
    off, ent, nfwd = oref.bucket_off().astype(np.int64), oref.entries(), oref.bucket_nfwd()
    exact = other = 0
    for b in np.flatnonzero(nfwd >= 48):
        e = np.asarray(ent[off[b]:off[b] + nfwd[b]]).astype(np.int64)
        assert len(e) >= N_COPIES, (b, len(e))
        if len(e) == N_COPIES and np.all(np.diff(e - np.asarray(pos)) == 0):
            exact += 1
        else:
            other += 1
    assert exact >= 40 and other <= 2, (exact, other)


@pytest.fixture(scope="module")
def world():
    g, unit, copies, pos = make_genome()
    return dict(fasta=td.fasta_text(g), unit=unit, copies=copies, pos=pos)


@pytest.mark.parametrize("v", [0, 2, 6])
def test_directed_reads_through_the_group_scan(v, world, oracle):
    copies, pos = world["copies"], world["pos"]
    kw = dict(s=16, v=v, I=4, S=1, r=1, n=0, f=5)
    reads = make_reads(world["unit"], v)
    check_claims(reads, world["unit"], copies, v)
    assert N_COPIES % 64 and N_COPIES % 256 and N_COPIES > 256
    oref = oracle.OracleRef(oracle.make_params(**kw), fasta_text=world["fasta"])
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_text=world["fasta"]).CreateIndex()
    try:
        check_buckets(oref, pos)
        exp, cnt = GB._expected(oracle, oref, "se", kw, reads, 0)
        for r, e in zip(reads, exp):   # the oracle says what the case says
            assert not e["filtered"], r["name"]
            if r["cls"][0] == "N" and e["pick"][0] == 0 and r["want"][0] == "hit":
                assert v == 0 and r["cls"] == "N0", r["name"]   # (-v 0 has one seed, and the reference's planner does not move it off an N in the read's first word: no hit)
            elif r["want"][0] == "hit":
                assert e["pick"][:2] == (len(PRISTINE), r["want"][1]) and e["pick"][3] in [pos[c] for c in PRISTINE], (r["name"], e["pick"])
                assert e["n_hit"][r["want"][1]] == len(PRISTINE) == sum(e["n_hit"]) + sum(e["n_chit"]), (r["name"], e["n_hit"], e["n_chit"])
            else:
                assert e["pick"][0] == 0 and sum(e["n_hit"]) + sum(e["n_chit"]) == 0, (r["name"], e["pick"])
        got = {}
        B.lib().bsx_set_heavy_threshold(48)
        try:
            for counters in (False, True):
                bt = B.SingleAlign(gref, len(reads), debug=True)
                try:
                    bt.set_work_counters(counters)
                    bt.ImportBatchReads([r["seq"] for r in reads], [r["qual"] for r in reads]).Do_Batch()
                    res = bt.results()
                    GB._compare("se", kw, reads, exp, bt, res, "counters %s" % counters)
                    c = bt.counters()
                    assert bt.heavy_units() > 0 and int(c[15]) > 0, (bt.heavy_units(), int(c[15]))   # hs_group ran: candidates evaluated in groups of two reads and more
                    if counters:
                        assert [int(x) for x in c[:4]] == cnt, ([int(x) for x in c[:4]], cnt)
                    got[counters] = tuple(a.tobytes() for a in res)
                finally:
                    bt.close()
        finally:
            B.lib().bsx_set_heavy_threshold(0)
        assert got[False] == got[True]
    finally:
        gref.close()
        oref.free()
