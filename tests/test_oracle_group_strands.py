"""Directed reads for k_hscan_same's groups on the reverse-strand copy, for pairs and at the ends of the reference: the constructions, with the oracle's word on
them.  CPU only; tests/test_gpu_group_strands.py imports this module and sends the same reads through the device.

The three directed group modules (tests/test_gpu_scan_word_order.py, test_gpu_offset_classes.py, test_gpu_group_cap.py) share one world: single-end ++ reads over
one chromosome with every copy of the unit deep inside random sequence — forward lists only, nowhere near an end.  Their genome builder, reads and checks are reused
here (WO.make_genome, WO.make_reads, WO.check_claims, OC._read, OC.first_heavy_list, GC.make_batch, GB._expected); what is new is where the copies stand.

WHAT DECIDES WHETHER A LIST IS SCANNED IN GROUPS.  The candidate list of one seed is the (phase x strand) sub-ranges of the index, the forward part of a bucket
first, its reverse part behind it (entries from bucket_nfwd on: positions on the reverse-strand copy, in that copy's coordinates).  The control pass cuts a list into
tasks on a grid of 8 192 candidates, and a run of sub-ranges shorter than that is ONE segment: a list of 421 forward and 421 reverse entries is one task that spans two
sub-ranges, and such a task is a group of one (it goes through the one-task path, which changes strand copy in its middle).  Only a task that lies inside one
sub-range can join a group.  A task's key is the index entry it starts at, and every entry belongs to exactly one strand part of one bucket, so two tasks of equal key
are on the same strand: a strand-0 and a strand-1 task can never share a key, whatever the genome.  The strand bit in k_task_groups' comparison of whole flags words
is therefore implied by the key, and the claim "tasks of equal key, length and offset that differ in strand do not merge" is not asserted anywhere below: it would be
vacuous.  What CAN occur, and is built here, is a strand-0 task and a strand-1 task of equal n (421), length and offset next to each other in one 64-slot segment of
the scan order (check_strand_neighbours): they differ in key and must stay two groups.

WORLD "strands" (the group path on the reverse copy).  chrR is WO.make_genome(77)'s chromosome, copies of unit U0 on the forward strand; chrM is the reverse
complement of WO.make_genome(78)'s, so the copies of its unit U1 stand on chrM's reverse strand.  Both lengths are multiples of 4 (spacers are multiples of 4, units
200, the tail 400), so a mirrored copy lies on the -I 4 grid again.  A read made from U0 has forward lists only, a read made from U1 reverse lists only (the index says
so: check_buckets_strands), each of the 421 copies.  ENTRY ORDER ON THE REVERSE COPY: the reverse copy of chrM is the reverse complement of chrM and its N pad — pad
letters first, then make_genome(78)'s chromosome as written — and entries are in ascending position of that copy: entry i of a reverse list is mirrored copy i, the
same order as on the forward strand, although in chrM's forward coordinates the copies run backwards.  So the four pristine copies (WO.PRISTINE) lie in the same places of
a reverse list as of a forward one: lanes 0 and 63 of a full chunk, lane 0 of the second step and the last lane of the partial chunk; nothing had to be reordered.  The
oracle reports a reverse hit in forward coordinates: copy i of U1, read unit[a : a + L], at chrM letter (len - pos_i - 200) + 200 - a - L, chromosome id 3.
WORLD "both" is what one would build first: chrM the reverse complement of chrR itself, every bucket of the copies 421 forward and 421 mirrored entries.  Every list
there spans two sub-ranges, so nothing of it reaches a group; it is kept as a small case of its own because the one-task path's change of strand copy inside a task is
reached by no other directed read, but counter 15 is not asked to be above 0 there.

Pairs run over "strands": a pair made from U0 (mate 1 unit[0:L] with its C kept, mate 2 the +- read of unit[200-L:200]; the fragment is the copy, insert 200) and
the same made from U1 (the fragment on chrM's reverse strand), each unit with a twin that differs in one C not kept.

WORLD "edges".  Three chromosomes; chr1 and chr2 carry copies of U0 on the forward strand, chr3 is the reverse complement of an arrangement of U1, so that U1's reads meet
it on the reverse copy.  Every copy stands at a multiple of 4 within its chromosome (in chr3: within the reverse copy too, the chromosome's length being a multiple of 16).
  chr1 begins with U0[64:] (a truncated pristine copy at letter 0) and ends with a whole pristine copy flush at its last letter;
  chr2 begins with a whole pristine copy at letter 0 and ends with U0[:136], flush;
  chr3's reverse copy begins with U1[64:] behind its N pad — the LAST letters of the LAST chromosome — and ends with a whole pristine copy: letter 0 of chr3.
Between the ends stand copies with clusters of C->T differences as in WO.CHUNK_SETS, two more pristine copies, and one fragment, U[0:76] beside a truncated head or U[124:200] beside a truncated tail, which gives the
seeds that the truncated copy lacks their entry back: every seed of the unit that can lie on the index grid is then one bucket of the same size (check_edge_buckets), and
the planner's order among a read's unspoiled seeds is segment order, as in the shared world.  The reads are GC.make_batch's: L = 132, -v 6, classes a = 0, 32 and 64 of 6
reads each, met at unit letter 64; and L = 144, a = 0 and 32, -v 2, met at letter 32.  At the truncated head one group then holds an a = 64 member whose candidate is letter 0
(a hit) and a = 0 and a = 32 members whose candidates lie 64 and 32 letters before the chromosome, the frame of all of them starting in the margin (chr1) or in the N
pad (chr3's reverse copy); at the truncated tail of chr2 the a = 0 member fits and the others stick out into the pad.
WHERE THE BOUNDS TEST ALONE REJECTS.  The packed reference holds A for every pad and margin letter of the forward copy (N packs as A; margins are zero words), and between two
chromosomes lie at least 32 pad letters, so a neighbour cannot supply the missing part of the unit.  "pack" reads are added that are exactly what the array holds:
  head of chr1:  A * 64 + U0[64:132] (a = 0) and A * 32 + U0[64:164] (a = 32): no counted difference against the margin and the truncated copy; rejected by the bounds test only;
  tail of chr2:  U0[32:136] + A * 28 (a = 32) and U0[64:136] + the 60 letters behind chr2 (a = 64: its pad and the first letters of chr3): the same behind chr2's last letter.
The first seeds of the head's reads are poly-A (no bucket), so their first heavy list is the shared one without any spoiled seed; the tail's a = 32 read carries one difference in
each of its first two seeds, as its class does.  On chr3's reverse copy the pad letters are the reverse
complement of N's packing — T — and a run of T is what a converted read holds anyway: T * 32 + U1[64:164] (a = 32) and, the pad being 32 letters, the reverse
complement of chr2's first 32 letters + T * 32 + U1[64:132] (a = 0) are built for the head there.  check_pack
counts their differences against the packed letters; check_edges asserts from the oracle's records that every edge has a read with a hit at the edge copy and a read of the
same window and pass without one."""
import numpy as np
import pytest

import bsx_testdata as td
import test_gpu_boundaries as GB
import test_gpu_group_cap as GC
import test_gpu_offset_classes as OC
import test_gpu_scan_word_order as WO

UNIT, N_COPIES, PRISTINE = WO.UNIT, WO.N_COPIES, WO.PRISTINE
WORD_LENGTHS = (144, 129, 100, 80)
KW = {v: dict(s=16, v=v, I=4, S=1, r=1, n=0, f=5) for v in (2, 6)}
KW_N1 = dict(KW[2], n=1)
KW_PE = dict(s=16, v=2, I=4, S=1, r=1, m=100, x=300, pairend=1)
PE_LENGTHS = (144, 100)


# ---- world "strands" and world "both" ---------------------------------------------------------------------------------------------------------------------------

def make_strand_world(both=False):
    """genome and, per strand s, the unit, the copies as the read sees them, their positions in the chromosome's forward coordinates and the oracle's chromosome id"""
    g0, u0, c0, p0 = WO.make_genome(77)
    g1, u1, c1, p1 = (g0, u0, c0, p0) if both else WO.make_genome(78)
    R, X = g0[0][1], g1[0][1]
    assert len(R) % 4 == 0 and len(X) % 4 == 0
    M = td.revcomp(X)
    mpos = [len(X) - p - UNIT for p in p1]                       # mirrored copy i in chrM's forward coordinates: they run backwards
    mirrored = [td.revcomp(M[p:p + UNIT]) for p in mpos]         # what a read of the reverse strand is compared with, read back from chrM's text
    assert mirrored == c1 and all(p % 4 == 0 for p in mpos)
    genome = [("chrR", R), ("chrM", M)]
    return dict(genome=genome, fasta=td.fasta_text(genome), unit=(u0, u1), copies=(c0, mirrored), pos=(p0, mpos), rcpos=p1, chr_id=(0, 3), both=both)


def check_buckets_strands(oref, w):
    """split at bucket_nfwd: a bucket of U0's copies is the 421 forward entries in position order and nothing else, a bucket of U1's the 421 mirrored copies in the SAME
    order (ascending position on the reverse copy) and no forward entry; in world "both" every bucket of the copies holds both parts"""
    off, ent, nfwd = oref.bucket_off().astype(np.int64), oref.entries(), oref.bucket_nfwd().astype(np.int64)
    an, rco, size = oref.anchor().astype(np.int64), oref.rc_offset().astype(np.int64), oref.chr_size().astype(np.int64)
    pad = int(rco[1] - size[1])                                   # the reverse copy of chrM begins with its N pad
    assert 32 <= pad < 48, pad
    fpos, rpos = np.asarray(w["pos"][0]) + an[0], np.asarray(w["rcpos"]) + an[1] + pad
    n_f = n_r = n_both = 0
    for b in np.flatnonzero(np.diff(off) >= 48):
        f, r = np.asarray(ent[off[b]:off[b] + nfwd[b]]).astype(np.int64), np.asarray(ent[off[b] + nfwd[b]:off[b + 1]]).astype(np.int64)
        ef = len(f) == N_COPIES and np.all(np.diff(f - fpos) == 0) and 0 <= f[0] - fpos[0] <= UNIT - 16
        er = len(r) == N_COPIES and np.all(np.diff(r - rpos) == 0) and 0 <= r[0] - rpos[0] <= UNIT - 16
        n_both += bool(ef and er and f[0] - fpos[0] == r[0] - rpos[0])
        n_f += bool(ef and len(r) == 0)
        n_r += bool(er and len(f) == 0)
    if w["both"]:
        assert n_both >= 40 and n_f == 0 and n_r == 0, (n_both, n_f, n_r)
    else:
        assert n_f >= 40 and n_r >= 40 and n_both == 0, (n_f, n_r, n_both)
    # the strand parts of all buckets are disjoint ranges of entries: a task's key (the entry it starts at) names its strand
    assert np.all(off[:-1] + nfwd <= off[1:]) and np.all(np.diff(off) >= 0)


def hit_loc(w, s, i, a, L):
    """where the oracle reports read unit[a : a + L] of strand s at copy i: (chromosome id, forward-strand letter)"""
    return (w["chr_id"][s], w["pos"][s][i] + (a if s == 0 else UNIT - a - L))


def word_reads(w, v, L):
    """WO.make_reads' cases (word k, first+last, N in word j, each with its twin) of one length, made from both units"""
    out = []
    for s in (0, 1):
        rs = [dict(r, name="s%d_%s" % (s, r["name"]), strand=s, a=0) for r in WO.make_reads(w["unit"][s], v) if r["L"] == L]
        WO.check_claims(rs, w["unit"][s], w["copies"][s], v)      # against chrR's copies and, letter by letter, against the reverse complement of chrM's
        out += rs
    return out


def check_word_records(w, reads, exp, v):
    """the oracle says what the cases say: four hits of the class at the pristine copies of the read's own strand — the reverse ones in chrM's forward coordinates —
    and none anywhere else"""
    for r, e in zip(reads, exp):
        assert not e["filtered"], r["name"]
        s = r["strand"]
        all_hits = sorted(h for per_w in e["lists"] for o in per_w for h in o)
        if r["want"][0] == "hit":
            want = sorted(hit_loc(w, t, i, 0, r["L"]) for t in ((0, 1) if w["both"] else (s,)) for i in PRISTINE)
            assert all_hits == want, (r["name"], all_hits, want)
            cls = r["want"][1]
            # (n_hit / n_chit tell the READ's orientation, not the reference strand: the strand copy is the low bit of a hit's chromosome id)
            assert e["n_hit"][cls] == len(want) == sum(e["n_hit"]) and sum(e["n_chit"]) == 0, (r["name"], e["n_hit"], e["n_chit"])
            assert e["pick"][:2] == (len(want), cls), (r["name"], e["pick"])
        else:
            assert all_hits == [] and e["pick"][0] == 0, (r["name"], e["pick"])


def n1_reads(w, L=144, v=2):
    """-n 1: the +- forms of the word cases (the reverse complement of the same read with its C kept: the read's complementary orientation is the ++ read) and the -- forms
    (td.directed_read over the same letters with the same placed differences, complete conversion)"""
    out = []
    for r in word_reads(w, v, L):
        u = w["unit"][r["strand"]][:L]
        n_at = tuple(i for i, c in enumerate(r["seq"]) if c == "N")
        assert r["seq"].replace("C", "T") == td.directed_read(u, "++", subs=r["subs"], n_at=n_at)
        out.append(dict(r, name=r["name"] + "_+-", seq=td.revcomp(r["seq"]), form="+-", fwd=r["seq"]))
        if r["name"].endswith("a"):
            out.append(dict(r, name=r["name"] + "_--", seq=td.directed_read(u, "--", subs=r["subs"], n_at=n_at), form="--"))
    return out


def check_n1_records(w, reads, exp, v=2):
    """with -n 1 both orientations of a read meet both strand copies under the one C/T rule, so a +- read is also compared as it stands, where some of its placed
    differences are T under C and not counted: a case may be a hit of a lower class than it was built for.  What holds for every read: its hits are the four pristine
    copies of its own unit or none, a case built as a hit is one, and a -- read is the hit of class v in its complementary orientation, or nothing, as its case says"""
    n = {"+-": 0, "--": 0}
    for r, e in zip(reads, exp):
        assert not e["filtered"] and e["plan"] is not None and e["cplan"] is not None, r["name"]
        hits = [h for per_w in e["lists"] for o in per_w for h in o]
        want = sorted(hit_loc(w, r["strand"], i, 0, r["L"])[1] for i in PRISTINE)
        assert hits == [] or (sorted(p for _, p in hits) == want and {c >> 1 for c, _ in hits} == {w["chr_id"][r["strand"]] >> 1}), (r["name"], hits)
        if r["want"][0] == "hit":
            assert hits, r["name"]
        if r["form"] == "--":
            assert (e["n_chit"][v] == len(PRISTINE) if r["want"][0] == "hit" else not hits) and sum(e["n_hit"]) == 0, (r["name"], e["n_hit"], e["n_chit"])
        else:   # the complementary plan (cplan) of a +- read is the ++ read's: it holds a list of the copies, which OC.first_heavy_list finds as in the forward plan
            seed, h = OC.first_heavy_list(dict(r, seq=r["fwd"]), w["unit"][r["strand"]], e["cplan"])
            assert seed is not None and seed % 4 == 0 and h == -seed, (r["name"], seed, h, e["cplan"])
        n[r["form"]] += bool(hits)
    assert n["+-"] >= 40 and n["--"] >= 20, n


def offset_batches(w):
    """one read per (strand, a): L = 144, a = 0 and 32 at -v 2 (met at unit letter 32) and L = 132, a = 0, 32 and 64 at -v 6 (met at 64), as within / over / N"""
    out = []
    for v, L, offs, meet in ((2, 144, (0, 32), 32), (6, 132, (0, 32, 64), 64)):
        for kind, n, n_at in (("within", v, ()), ("over", v + 1, ()), ("N", v, (L - 2,))):
            reads = [dict(OC._read(w["unit"][s], L, a, n, (meet - a) // 16, n_at=n_at, tag="%s_s%d" % (kind, s)), strand=s) for s in (0, 1) for a in offs]
            out.append(dict(name="offsets L%d -v %d %s" % (L, v, kind), v=v, kind=kind, meet=meet, reads=reads))
    return out


def cap_batches(w):
    """a class of 65 reads, and 40 + 30 in two classes, from GC.make_batch, on each strand: the second ballot of k_task_groups and the frame's move before the last row"""
    out = []
    for sizes in ((65,), (40, 30)):
        for kind in ("plain", "over", "N"):
            reads = [dict(r, name="s%d_%s" % (s, r["name"]), strand=s) for s in (0, 1) for r in GC.make_batch(w["unit"][s], 144, 2, sizes, kind)]
            out.append(dict(name="cap %s %s" % (sizes, kind), v=2, kind=kind, meet=32, reads=reads))
    return out


def first_lists(w, reads, exp, which="plan"):
    """(unit letter, read offset) of every read's first heavy list under the oracle's plan"""
    return [OC.first_heavy_list(r, w["unit"][r["strand"]], e[which]) for r, e in zip(reads, exp)]


def check_meet(w, b, exp, which="plan"):
    """the construction holds under the oracle's planner: every read's first heavy list is the shared seed's, with the offset of its class"""
    fh = first_lists(w, b["reads"], exp, which)
    assert fh == [(b["meet"], r["a"] - b["meet"]) for r in b["reads"]], (b["name"], fh)


def check_strand_neighbours(b):
    """a strand-0 and a strand-1 read of equal length and offset in the same batch: their first tasks are of equal n (the copies), length and offset, and differ in key"""
    keys = {(r["strand"], r["L"], r["a"]) for r in b["reads"]}
    assert any((1 - s, L, a) in keys for s, L, a in keys), b["name"]


def check_picks(w, b, exp):
    for r, e in zip(b["reads"], exp):
        assert not e["filtered"], r["name"]
        hits = [h for per_w in e["lists"] for o in per_w for h in o]
        if "over" in r["name"]:
            assert e["pick"][0] == 0 and hits == [], (r["name"], e["pick"])                  # one difference too many
        else:
            assert e["pick"][0] >= len(PRISTINE), (r["name"], e["pick"])
            assert {hit_loc(w, r["strand"], i, r["a"], r["L"]) for i in PRISTINE} <= set(hits), (r["name"], hits)
            assert all(c == w["chr_id"][r["strand"]] for c, _ in hits), (r["name"], hits)   # a read of U1 on the reverse strand of chrM only


# ---- pairs -------------------------------------------------------------------------------------------------------------------------------------------------------

def _kept(u, subs=(), n_at=(), drop=()):
    """the letters u as a read with its C kept: G <-> A at subs, N at n_at, the C at drop not kept"""
    assert all(u[i] in "GA" for i in subs) and all(u[i] == "C" for i in drop)
    return "".join("N" if i in n_at else ("A" if c == "G" else "G") if i in subs else "T" if i in drop else c for i, c in enumerate(u))


def pair_cases(w, L):
    """the pairs of one mate length, -v 2: (case, differences of mate 1, of mate 2 — in the letters of the fragment's strand —, N of mate 2, what it must be)"""
    v, out = KW_PE["v"], []
    kl = WO.LAST_EVALUATED[L]
    for s in (0, 1):
        unit = w["unit"][s]
        t1, t2 = unit[:L], unit[UNIT - L:]
        car = lambda t, k: WO._at(t, 32 * k, 32 * k + 32, "GA")
        last2 = (L - 1) // 32
        cases = [("pristine", (), (), (), "pair"),
                 ("m1", car(t1, 1)[:v], (), (), "pair"), ("m2", (), car(t2, 1)[:v], (), "pair"),
                 ("both_first", car(t1, 0)[:v], car(t2, 0)[:v], (), "pair"), ("both_last", car(t1, kl)[:v], car(t2, kl)[:v], (), "pair"),
                 ("over1", car(t1, 0)[:v] + car(t1, kl)[-1:], (), (), "b_only"), ("over2", (), car(t2, 0)[:v] + car(t2, kl)[-1:], (), "a_only"),
                 ("N2", (), car(t2, 0)[:v], (min(32 * last2 + 12, L - 1),), "pair")]
        for name, s1, s2, n2, want in cases:
            c1 = [i for i in WO._at(t1, 48, L, "C") if i not in s1][:1]
            c2 = [i for i in WO._at(t2, 0, L - 48, "C") if i not in s2 and i not in n2][:1]
            for tw, d1, d2 in (("a", (), ()), ("b", c1, c2)):
                m1, f2 = _kept(t1, s1, (), d1), _kept(t2, s2, n2, d2)
                assert sum(map(WO._counted, m1, t1)) == len(s1) and sum(map(WO._counted, f2, t2)) == len(s2)
                out.append(dict(name="s%d_L%d_%s_%s" % (s, L, name, tw), seq1=m1, qual1="I" * L, seq2=td.revcomp(f2), qual2="I" * L, strand=s, L=L, case=name, want=want,
                                n1=len(s1), n2=len(s2), fwd2=f2))
    assert len({(p["seq1"], p["seq2"]) for p in out}) == len(out)
    return out


def check_pair_records(w, pairs, exp):
    """four pairs at the pristine copies, insert 200, where both mates are within -v; where one carries v + 1 the unit is unpaired and the other mate keeps its own hits:
    every copy within -v of it, counted letter by letter (mate 2 covers unit[200 - L:], where the copies whose clusters lie in the unit's first words are pristine too)"""
    v = KW_PE["v"]
    for p, e in zip(pairs, exp):
        s, L = p["strand"], p["L"]
        assert not e["a"]["filtered"] and not e["b"]["filtered"], p["name"]
        hits = {m: sorted(h for per_w in e[m]["lists"] for o in per_w for h in o) for m in "ab"}
        at = lambda a: sorted(hit_loc(w, s, i, a, L) for i in PRISTINE)
        if p["want"] == "pair":
            assert e["paired"] > 0 and not e["unpaired_out"], (p["name"], e["paired"])
            assert sum(e["n_pairs"]) == len(PRISTINE) == e["n_pairs"][p["n1"] + p["n2"]], (p["name"], e["n_pairs"])
            prs = [q for per_w in e["pairs"] for q in per_w]
            assert sorted((q[4], q[5]) for q in prs) == at(0) and sorted((q[6], q[7]) for q in prs) == at(UNIT - L) and all(q[3] == UNIT for q in prs), (p["name"], prs)
        else:
            assert e["paired"] == 0 and e["unpaired_out"] and sum(e["n_pairs"]) == 0, (p["name"], e["paired"], e["n_pairs"])
            ok, bad = ("b", "a") if p["want"] == "b_only" else ("a", "b")
            seq, a = (p["fwd2"], UNIT - L) if ok == "b" else (p["seq1"], 0)
            near = [i for i, t in enumerate(w["copies"][s]) if WO._counted(seq, t[a:a + L]) <= v]
            assert set(PRISTINE) <= set(near) and hits[bad] == [] and hits[ok] == sorted(hit_loc(w, s, i, a, L) for i in near), (p["name"], hits)
            assert e[ok]["pick"][:2] == (sum(1 for i in near if WO._counted(seq, w["copies"][s][i][a:a + L]) == 0), 0), (p["name"], e[ok]["pick"])


# ---- world "edges" -----------------------------------------------------------------------------------------------------------------------------------------------

N_MID = 70          # copies with clusters between the ends of an arrangement: with the ends, the pristine copies and the fragments a list holds 76 or 77 entries — two chunks


def _arrangement(unit, rng, head, tail):
    """one chromosome's worth: `head` flush at letter 0, `tail` flush at the end, between them N_MID copies with C->T clusters (WO.CHUNK_SETS' sets in turn), two pristine
    copies and, where an end is truncated, the fragment unit[0:76] or unit[124:200]; every whole copy and both ends' unit letter 0 at a multiple of 4.  Returns (text, [(position of unit letter 0,
    first and last unit letter present, pristine)])"""
    sp = lambda: td.random_seq(rng, 4 * int(rng.integers(50, 100)), 0.5).tobytes().decode()
    parts, places, at = [], [], 0

    def put(text, lo, hi, pristine):
        nonlocal at
        parts.append(text)
        places.append((at - lo, lo, hi, pristine))
        at += len(text)

    def gap():
        nonlocal at
        s = sp()
        parts.append(s)
        at += len(s)

    put(unit[head[0]:head[1]], head[0], head[1], True)
    for c in range(N_MID):
        gap()
        if c in (N_MID // 3, 2 * N_MID // 3):
            put(unit, 0, UNIT, True)
            gap()
        if c == 5 and head[0]:      # the fragment that gives the seeds a truncated end lacks their entry back
            put(unit[0:76], 0, 76, True)
            gap()
        if c == 5 and tail[1] < UNIT:
            put(unit[124:UNIT], 124, UNIT, True)
            gap()
        t = list(unit)
        for k in WO.SETS[c % len(WO.SETS)]:
            for i in rng.choice(WO._at(unit, *WO.WORD[k], "C"), WO.CLUSTER, replace=False):
                t[int(i)] = "T"
        put("".join(t), 0, UNIT, False)
    gap()
    put(unit[tail[0]:tail[1]], tail[0], tail[1], True)
    text = "".join(parts)
    assert all((p + lo) % 4 == 0 for p, lo, _, _ in places)
    return text, places


def make_edge_world(seed=91):
    rng = np.random.default_rng(seed)
    _, u0, _, _ = WO.make_genome(77)
    _, u1, _, _ = WO.make_genome(78)
    c1, p1 = _arrangement(u0, rng, (64, UNIT), (0, UNIT))
    c2, p2 = _arrangement(u0, rng, (0, UNIT), (0, 136))
    while True:   # chr3's length a multiple of 16 (one draw in four): its reverse copy then begins with whole pad words, and the grid of the copy is the arrangement's
        x3, p3 = _arrangement(u1, rng, (64, UNIT), (0, UNIT))
        if len(x3) % 16 == 0:
            break
    assert len(c1) % 4 == 0 and len(c2) % 4 == 0
    for text, pl in ((c1, p1), (c2, p2), (x3, p3)):       # the ends are flush: first letter and last letter of the chromosome
        assert pl[0][0] + pl[0][1] == 0 and pl[-1][0] + pl[-1][2] == len(text)
    genome = [("chr1", c1), ("chr2", c2), ("chr3", td.revcomp(x3))]
    return dict(genome=genome, fasta=td.fasta_text(genome), unit=(u0, u1), places=((0, p1), (1, p2), (2, p3)), x3=x3,
                edges=dict(head1=(0, p1[0]), tail1=(0, p1[-1]), head2=(1, p2[0]), tail2=(1, p2[-1]), head3=(2, p3[0]), tail3=(2, p3[-1])))


def edge_hit(w, edge, a, L):
    """(chromosome id, forward letter) at which read unit[a : a + L] would be reported at the edge's copy, and whether it lies inside the chromosome"""
    ci, (p, lo, hi, _) = w["edges"][edge]
    start = p + a                                          # in the arrangement's own direction
    inside = lo <= a and a + L <= hi
    if ci < 2:
        return (2 * ci, start), inside
    return (2 * ci + 1, len(w["x3"]) - start - L), inside                # chr3 is the reverse complement of the arrangement


def check_edge_buckets(oref, w):
    """every seed of a unit that can lie on the grid is one bucket of the same size — all its copies, whole, truncated or fragment — and on one strand only"""
    off, nfwd = oref.bucket_off().astype(np.int64), oref.bucket_nfwd().astype(np.int64)
    tot = np.diff(off)
    n0 = len(w["places"][0][1]) + len(w["places"][1][1]) - 2       # per seed: every place of chr1 and chr2 but, in each, the truncated copy or the fragment that lacks it
    n1 = len(w["places"][2][1]) - 1
    big = np.flatnonzero(tot >= 48)
    f_only, r_only = big[(nfwd[big] == tot[big])], big[nfwd[big] == 0]
    assert np.sum(tot[f_only] == n0) >= 40 and np.sum(tot[r_only] == n1) >= 40, (n0, n1, sorted(tot[big]))
    assert n0 >= 128 and n1 >= 65                                  # more than a chunk of 64 candidates on either strand


def edge_pack_reads(w):
    """reads that are exactly what the packed reference holds outside the chromosome (see the module text); L = 132, -v 6, window of unit letter 64"""
    u0, u1 = w["unit"]
    L = 132
    mk = lambda name, s, a, seq, edge, spoiled=0: dict(name=name, seq=seq, qual="I" * L, L=L, a=a, strand=s, edge=edge, pack=True, spoiled=spoiled)

    def spoil(t, n):   # one difference in each of the first n seeds, where OC._read places it: the shared seed's list is then the first that goes to the scan kernel
        t = list(t)
        for j in range(n):
            k = [16 * j + k for k in (12, 13, 11, 10, 9, 8) if t[16 * j + k] in "GA"][0]
            t[k] = "A" if t[k] == "G" else "G"
        return "".join(t)
    keep = lambda t: t                                             # the unit's letters with their C kept
    c2, c3 = w["genome"][1][1], w["genome"][2][1]
    nxt = "A" * (32 + (-len(c2)) % 16) + c3                        # what the packed forward copy holds behind chr2's last letter: its pad, then chr3
    out = [mk("pack_head1_a0", 0, 0, "A" * 64 + keep(u0[64:132]), "head1"), mk("pack_head1_a32", 0, 32, "A" * 32 + keep(u0[64:164]), "head1"),
           mk("pack_tail2_a32", 0, 32, spoil(u0[32:136], 2) + "A" * 28, "tail2", 2), mk("pack_tail2_a64", 0, 64, keep(u0[64:136]) + nxt[:60], "tail2"),
           mk("pack_head3_a0", 1, 0, td.revcomp(c2[:32]) + "T" * 32 + keep(u1[64:132]), "head3"), mk("pack_head3_a32", 1, 32, "T" * 32 + keep(u1[64:164]), "head3")]
    assert all(len(r["seq"]) == L for r in out)
    return out


def check_pack(oref, w, reads):
    """no counted difference between a pack read and the packed letters at its place that sticks out of the chromosome but the ones placed to spoil its first seeds, fewer
    than -v 6 allows: the bounds test is what rejects it"""
    an, size, rco = oref.anchor().astype(np.int64), oref.chr_size().astype(np.int64), oref.rc_offset().astype(np.int64)
    letters = lambda words, p, n: "".join("ACGT"[(int(words[q // 16]) >> (30 - 2 * (q % 16))) & 3] for q in range(p, p + n))
    for r in reads:
        ci, (p, lo, hi, _) = w["edges"][r["edge"]]
        if r["strand"] == 0:
            got = letters(oref.refcat(), int(an[ci]) + p + r["a"], r["L"])
        else:
            got = letters(oref.crefcat(), int(an[ci]) + int(rco[ci] - size[ci]) + p + r["a"], r["L"])
        assert WO._counted(r["seq"], got) == r["spoiled"] <= 6, (r["name"], r["seq"], got)
        assert not (lo <= r["a"] and r["a"] + r["L"] <= hi)


def edge_batches(w):
    """GC.make_batch's classes on both strands: L = 132, -v 6, 6 + 6 + 6 met at unit letter 64 (with the pack reads), and L = 144, -v 2, 6 + 6 met at letter 32"""
    out = []
    for v, L, sizes, meet in ((6, 132, (6, 6, 6), 64), (2, 144, (6, 6), 32)):
        for kind in ("plain", "over", "N"):
            reads = [dict(r, name="s%d_%s" % (s, r["name"]), strand=s) for s in (0, 1) for r in GC.make_batch(w["unit"][s], L, v, sizes, kind)]
            pack = edge_pack_reads(w) if L == 132 and kind == "plain" else []
            out.append(dict(name="edges L%d -v %d %s" % (L, v, kind), v=v, kind=kind, meet=meet, reads=reads + pack))
    return out


def check_edges(w, b, exp):
    """from the oracle's records: at every edge a read of the batch has a hit at the edge's copy and a read of the same window and pass (its first heavy list is the shared
    seed's: check_meet) has its candidate there outside the chromosome and no hit; a pack read is never a hit anywhere"""
    inside, outside = set(), set()
    for r, e in zip(b["reads"], exp):
        hits = {h for per_w in e["lists"] for o in per_w for h in o}
        if r.get("pack"):
            assert e["pick"][0] == 0 and not hits, (r["name"], hits)
        for edge, (ci, _) in w["edges"].items():
            if (ci == 2) != (r["strand"] == 1):
                continue
            at, ins = edge_hit(w, edge, r["a"], r["L"])
            if ins and "over" not in r["name"] and not r.get("pack"):
                assert at in hits, (r["name"], edge, at, sorted(hits))
                inside.add(edge)
            if not ins:
                assert at not in hits, (r["name"], edge, at)
                outside.add(edge)
    truncated = {"head1", "tail2", "head3"}
    # (a read of 144 letters fits no truncated copy: there every member of its groups sticks out, and the hits are at the whole copies flush with an end)
    assert inside == (set(w["edges"]) if b["meet"] == 64 else set(w["edges"]) - truncated) and outside == truncated, (b["name"], inside, outside)


# ---- the tests: the constructions under the oracle ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def strands(oracle):
    w = make_strand_world()
    w["oref"] = {v: oracle.OracleRef(oracle.make_params(**KW[v]), fasta_text=w["fasta"]) for v in (2, 6)}
    yield w
    for o in w["oref"].values():
        o.free()


@pytest.fixture(scope="module")
def edges(oracle):
    w = make_edge_world()
    w["oref"] = {v: oracle.OracleRef(oracle.make_params(**KW[v]), fasta_text=w["fasta"]) for v in (2, 6)}
    yield w
    for o in w["oref"].values():
        o.free()


def test_index_of_the_strand_worlds(strands, oracle):
    check_buckets_strands(strands["oref"][2], strands)
    w = make_strand_world(both=True)
    oref = oracle.OracleRef(oracle.make_params(**KW[2]), fasta_text=w["fasta"])
    try:
        check_buckets_strands(oref, w)
    finally:
        oref.free()


@pytest.mark.parametrize("v", [2, 6])
def test_word_cases_on_both_strands(v, strands, oracle):
    for L in WORD_LENGTHS:
        reads = word_reads(strands, v, L)
        assert 40 <= len(reads) < 200
        exp, _ = GB._expected(oracle, strands["oref"][v], "se", KW[v], reads, 0)
        check_word_records(strands, reads, exp, v)
        assert all(e["cplan"] is None for e in exp)                   # -n 0: one orientation of the read; its reverse lists are the reverse part of the same plan's buckets


def test_word_cases_with_both_orientations(strands, oracle):
    oref = oracle.OracleRef(oracle.make_params(**KW_N1), fasta_text=strands["fasta"])
    try:
        reads = n1_reads(strands)
        exp, _ = GB._expected(oracle, oref, "se", KW_N1, reads, 0)
        check_n1_records(strands, reads, exp)
    finally:
        oref.free()


def test_offset_classes_and_caps_on_both_strands(strands, oracle):
    for b in offset_batches(strands) + cap_batches(strands):
        exp, _ = GB._expected(oracle, strands["oref"][b["v"]], "se", KW[b["v"]], b["reads"], 0)
        check_meet(strands, b, exp)
        check_strand_neighbours(b)
        check_picks(strands, b, exp)


def test_both_strands_in_one_list(oracle):
    w = make_strand_world(both=True)
    oref = oracle.OracleRef(oracle.make_params(**KW[2]), fasta_text=w["fasta"])
    try:
        reads = [r for r in word_reads(w, 2, 144) if r["strand"] == 0]
        exp, _ = GB._expected(oracle, oref, "se", KW[2], reads, 0)
        check_word_records(w, reads, exp, 2)
    finally:
        oref.free()


def test_pairs_on_both_strands(strands, oracle):
    oref = oracle.OracleRef(oracle.make_params(**KW_PE), fasta_text=strands["fasta"])
    try:
        for L in PE_LENGTHS:
            pairs = pair_cases(strands, L)
            exp, _ = GB._expected(oracle, oref, "pe", KW_PE, pairs, 0)
            check_pair_records(strands, pairs, exp)
    finally:
        oref.free()


def test_groups_at_the_edges_of_the_reference(edges, oracle):
    check_edge_buckets(edges["oref"][2], edges)
    check_pack(edges["oref"][6], edges, edge_pack_reads(edges))
    for b in edge_batches(edges):
        exp, _ = GB._expected(oracle, edges["oref"][b["v"]], "se", KW[b["v"]], b["reads"], 0)
        check_meet(edges, b, exp)
        check_strand_neighbours(b)
        check_edges(edges, b, exp)
