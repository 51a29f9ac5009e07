"""All hits (include/bsx.h: bsx_batch_set_all_hits): the best class's whole list of every multi-mapped read or pair, kept by a production-mode
batch (debug off, per-wave slabs) in the all-hits pool.  Needs an MI355X.

Against the goldens (every list of every class as the real reference produced them), for every golden set with -r 1:
  * the lists rebuilt from the spans equal the golden's best-class lists, order included; units that have nothing to add have empty spans; the
    number of emitting units is the one counted on the CPU from the goldens (so a filter that skips everything fails);
  * records and class counts are byte-identical to a run of the same batch without a pool;
  * entry myrand(index) % n of every span is the record's own placement;
  * the spans' words add up to the need the library reports, no two spans overlap, nothing is dropped.
Units whose reference result depends on the read before them (tests/test_gpu_parity.py: _leaky) are compared with the oracle instead of the golden,
as the parity suite does; none of them emits in the golden sets.
The third kind of emission (mates of an unreported pair) does not occur in the goldens' own pairs: c3_pe150 with the mates crossed — mate 1 of
pair i with mate 2 of pair (i + 150) % 300 — leaves 298 pairs unreported, 4 of their mates multi-mapped; expected lists from the oracle.
Exact mode (bsx_batch_set_leak_exact): the goldens' lists for EVERY unit, the call-order dependent ones included.
Overflow: a pool of a quarter of the need drops units, keeps their counts, leaves every other span right and the records untouched; the reported
need then holds everything."""
import numpy as np
import pytest

import bsmap_amd as B
import golden_util as G

pytestmark = pytest.mark.gpu

# set -> (emitting units, longest list): counted on the CPU from tests/golden/*.json.gz
EMITTING = {"c1_se36": (28, 1000), "c2_se100": (7, 616), "c2_se100_n1": (6, 622), "c4_rrbs75": (1, 2), "c3_pe150": (4, 205), "c5_trim_pe150": (7, 1000)}
POOL = 1 << 20   # words: far above what 440 units can want (28 lists of at most 1064 placements)


def myrand(index, randseed):
    """bsx_myrand (bsmap_amd/csrc/bsx_dev.h), the reference's pick among equal-best hits"""
    m = (1 << 64) - 1
    def s32(x):
        x &= 0xffffffff
        return x - (1 << 32) if x & 0x80000000 else x
    v = ((s32(index) + s32(randseed * 1000000)) * 3935559000370003845 + 2691343689449507681) & m
    v ^= v >> 21; v ^= (v << 37) & m; v ^= v >> 4
    v = (v * 4768777513237032717) & m
    v ^= (v << 20) & m; v ^= v >> 41; v ^= (v << 5) & m
    return v & 0xffffffff


def _leaky(length, kw):
    if "D" in kw:
        return False
    return (length - kw.get("I", 4) + 1) % kw.get("s", 16) == 0


def _best(n_hit, n_chit, nclass):
    for w in range(nclass):
        if n_hit[w] + n_chit[w]:
            return w, n_hit[w] + n_chit[w]
    return None


def oracle_se_lists(al, o):
    """what a single read emits, from the oracle's state after al.se(): (hits, [], [])"""
    if o.filtered or o.n_best < 2:
        return [], [], []
    w = o.best_class
    return al.se_hits(0, w, o.n_hit[w]) + al.se_hits(1, w, o.n_chit[w]), [], []


def oracle_pe_lists(al, o):
    """what a pair emits, from the oracle's state after al.pe()"""
    if not (o.tmp == 1 or o.paired == 0):
        return [], [], (al.pe_pairs(o.pair_class, o.pair_n) if o.pair_n >= 2 else [])
    out = []
    for mate, om in enumerate((o.a, o.b)):
        if om.filtered or om.n_best < 2:
            out.append([])
        else:
            w = om.best_class
            out.append(al.pe_hits(mate, 0, w, om.n_hit[w]) + al.pe_hits(mate, 1, w, om.n_chit[w]))
    return out[0], out[1], []


def golden_lists(e, kind, nclass):
    if kind == "se":
        b = None if e["filtered"] else _best(e["n_hit"], e["n_chit"], nclass)
        if not b or b[1] < 2:
            return [], [], []
        return [tuple(x) for x in e["hits"][b[0]][0]] + [tuple(x) for x in e["hits"][b[0]][1]], [], []
    if e["paired"] > 0 and e["tmp"] == 0:
        w = [k for k, n in enumerate(e["n_pairs"]) if n][0]
        return [], [], ([tuple(x) for x in e["pairs"][w]] if e["n_pairs"][w] >= 2 else [])
    out = []
    for m in "ab":
        b = None if e[m]["filtered"] else _best(e[m]["n_hit"], e[m]["n_chit"], nclass)
        out.append([] if not b or b[1] < 2 else [tuple(x) for x in e[m]["hits"][b[0]][0]] + [tuple(x) for x in e[m]["hits"][b[0]][1]])
    return out[0], out[1], []


def check_spans(al, spans, pool, expect_dropped=0):
    """the invariants of a run's spans: words add up to the need, live spans lie inside the pool and do not overlap"""
    need, dropped = al.all_hits_need()
    words = spans["n"].astype(np.int64) * np.array([2, 2, 6])
    assert int(words.sum()) == need, (int(words.sum()), need)
    live = (spans["n"] > 0) & (spans["off"] != B.SPAN_DROPPED)
    gone = (spans["n"] > 0) & (spans["off"] == B.SPAN_DROPPED)
    assert int(gone.any(axis=1).sum()) == dropped, (int(gone.any(axis=1).sum()), dropped)
    assert (dropped > 0) == bool(expect_dropped), dropped
    if not dropped:
        assert len(pool) == need
    lo = spans["off"][live].astype(np.int64)
    hi = lo + words[live]
    order = np.argsort(lo)
    assert (hi <= len(pool)).all() and (lo[order][1:] >= hi[order][:-1]).all(), "spans overlap or leave the pool"
    assert (spans["n_fwd"] <= spans["n"]).all() and (spans["n_fwd"][:, 2] == 0).all()
    return need, dropped


def check_picks(kind, res, spans, pool, randseed, first_index=0):
    """entry myrand(index) % n of every live span is the record's own placement; entries from n_fwd on are the ones with BSX_F_CHAIN"""
    checked = 0
    for i in range(len(spans)):
        la, lb, lp = B.all_hits_lists(spans[i], pool)
        j_of = lambda n: myrand(first_index + i, randseed) % n
        if kind == "se":
            recs = [(res[0][i], la, spans[i][0])]
        else:
            g = res[0][i]
            if lp:
                j = j_of(len(lp))
                assert lp[j] == (g["chain"], g["na"], g["nb"], g["insert"], g["a_chr"], g["a_loc"], g["b_chr"], g["b_loc"]), i
                assert len(lp) == g["n_pairs"] and not g["unpaired_out"], i
                checked += 1
            recs = [(g["a"], la, spans[i][0]), (g["b"], lb, spans[i][1])] if g["unpaired_out"] else []
        for h, lst, sp in recs:
            if not lst:
                continue
            j = j_of(len(lst))
            assert len(lst) == h["n_best"] and lst[j] == (h["chr"], h["loc"]), i
            assert (j >= sp["n_fwd"]) == bool(h["flags"] & B.F_CHAIN), i
            checked += 1
    return checked


def _run_twice(al, pool_words=POOL):
    """production-mode run without a pool, then the same batch with one: (records without, records with, spans, pool)"""
    al.Do_Batch()
    plain = tuple(None if x is None else x.copy() for x in al.results())
    al.set_all_hits(pool_words)
    al.Do_Batch()
    withp = al.results()
    for a, b in zip(plain, withp):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), "a pool changed the records"
    spans, pool = al.all_hits()
    return plain, spans, pool


def _load_batch(meta, gref, reads=None):
    reads = reads or meta["reads"]
    if meta["kind"] == "se":
        al = B.SingleAlign(gref, len(reads))
        al.ImportBatchReads([r["seq"] for r in reads], [r["qual"] for r in reads])
    else:
        al = B.PairAlign(gref, len(reads))
        al.ImportBatchReads([r["seq1"] for r in reads], [r["seq2"] for r in reads], [r["qual1"] for r in reads], [r["qual2"] for r in reads])
    return al


@pytest.fixture(scope="module", params=sorted(EMITTING))
def case(request, oracle):
    meta, arr, fasta = G.load(request.param)
    kw = meta["kw"]
    assert kw.get("r", 1) == 1
    oref = oracle.OracleRef(oracle.make_params(**kw), fasta_path=fasta)
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_path=fasta).CreateIndex()
    yield request.param, meta, oref, gref, oracle
    gref.close()
    oref.free()


def test_golden_lists_in_production_mode(case):
    name, meta, oref, gref, O = case
    kw, kind = meta["kw"], meta["kind"]
    nclass = kw["v"] + 1
    al = _load_batch(meta, gref)
    oal = O.OracleAligner(oref, leak_mode=0)
    try:
        res, spans, pool = _run_twice(al)
        need, _ = check_spans(al, spans, pool)
        emitting, longest, from_oracle = 0, 0, 0
        for i, (r, e) in enumerate(zip(meta["reads"], meta["expected"])):
            got = B.all_hits_lists(spans[i], pool)
            lens = [e["len"]] if kind == "se" else [e["a"]["len"], e["b"]["len"]]
            filt = e["filtered"] if kind == "se" else (e["a"]["filtered"] or e["b"]["filtered"])
            if filt or any(_leaky(x, kw) for x in lens):   # the golden is call-order dependent (or holds no lists) there: the oracle from zeroed state
                want = oracle_se_lists(oal, oal.se(i, r["seq"], r["qual"])) if kind == "se" else oracle_pe_lists(oal, oal.pe(i, r["seq1"], r["seq2"], r["qual1"], r["qual2"]))
                from_oracle += 1
            else:
                want = golden_lists(e, kind, nclass)
            assert got == tuple(want), (name, i)
            if any(want):
                emitting += 1
                longest = max([longest] + [len(x) for x in want])
        print(f"{name}: {emitting} emitting units of {len(spans)}, longest list {longest}, {need} words, {from_oracle} units compared with the oracle instead of the golden")
        assert (emitting, longest) == EMITTING[name]
        assert check_picks(kind, res, spans, pool, kw.get("S", 0)) == emitting
    finally:
        oal.free()
        al.close()


def test_mates_of_unreported_pairs(oracle):
    """c3_pe150 with the mates crossed: 298 of 300 pairs unreported, 4 of their mates with two or more best hits (the longest list 404)"""
    meta, arr, fasta = G.load("c3_pe150")
    kw = meta["kw"]
    rd = meta["reads"]
    reads = [dict(seq1=rd[i]["seq1"], qual1=rd[i]["qual1"], seq2=rd[(i + 150) % 300]["seq2"], qual2=rd[(i + 150) % 300]["qual2"]) for i in range(300)]
    oref = oracle.OracleRef(oracle.make_params(**kw), fasta_path=fasta)
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_path=fasta).CreateIndex()
    oal = oracle.OracleAligner(oref, leak_mode=0)
    al = _load_batch(meta, gref, reads)
    try:
        want, unreported = [], 0
        for i, r in enumerate(reads):
            o = oal.pe(i, r["seq1"], r["seq2"], r["qual1"], r["qual2"])
            unreported += bool(o.tmp == 1 or o.paired == 0)
            want.append(tuple(oracle_pe_lists(oal, o)))
        mates = [l for w in want for l in w[:2] if l]
        assert unreported == 298 and len(mates) == 4 and max(len(l) for l in mates) == 404, (unreported, [len(l) for l in mates])
        res, spans, pool = _run_twice(al)
        check_spans(al, spans, pool)
        for i in range(300):
            assert B.all_hits_lists(spans[i], pool) == want[i], i
        assert int(res[0]["unpaired_out"].sum()) == 298
        assert check_picks("pe", res, spans, pool, kw.get("S", 0)) == 4 + sum(1 for w in want if w[2])
    finally:
        al.close()
        oal.free()
        gref.close()
        oref.free()


def test_overflow_drops_whole_units_and_reports_the_need(oracle):
    """c1_se36 (28 emitting reads, 1 000-hit lists) with a pool of a quarter of the need: an ordinary capacity path"""
    meta, arr, fasta = G.load("c1_se36")
    kw = meta["kw"]
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_path=fasta).CreateIndex()
    al = _load_batch(meta, gref)
    try:
        res, spans, pool = _run_twice(al)
        need, _ = check_spans(al, spans, pool)
        full = [B.all_hits_lists(spans[i], pool) for i in range(len(spans))]
        al.set_all_hits(need // 4)
        al.Do_Batch()
        for a, b in zip(res, al.results()):
            assert a.tobytes() == b.tobytes(), "a full pool changed the records"
        s2, p2 = al.all_hits()
        need2, dropped = check_spans(al, s2, p2, expect_dropped=1)
        assert need2 == need and 0 < dropped < 28 and len(p2) <= need // 4
        assert np.array_equal(s2["n"], spans["n"]) and np.array_equal(s2["n_fwd"], spans["n_fwd"]), "a dropped span lost its counts"
        kept = 0
        for i in range(len(s2)):
            got = B.all_hits_lists(s2[i], p2)
            if got[0] is None:
                continue
            assert got == full[i], i
            kept += bool(got[0])
        assert kept == 28 - dropped
        al.set_all_hits(need2)   # what the library said it needs, not a word more
        al.Do_Batch()
        s3, p3 = al.all_hits()
        assert check_spans(al, s3, p3) == (need, 0)
        assert [B.all_hits_lists(s3[i], p3) for i in range(len(s3))] == full
        al.set_all_hits(0)       # detached: the calls say so, the batch runs on
        with pytest.raises(B.BsxError):
            al.all_hits_need()
        al.Do_Batch()
        assert al.results()[0].tobytes() == res[0].tobytes()
    finally:
        al.close()
        gref.close()


def test_needs_report_repeat_hits_1():
    meta, arr, fasta = G.load("c2_se100_r0_w3")
    gref = B.RefSeq(B.make_params(**meta["kw"])).Run_ConvertBinseq(fasta_path=fasta).CreateIndex()
    al = B.SingleAlign(gref, 16)
    try:
        with pytest.raises(B.BsxError) as e:
            al.set_all_hits(1024)
        assert e.value.code == -1
        al.set_all_hits(0)   # detaching nothing is fine
    finally:
        al.close()
        gref.close()


def test_run_range_fills_the_spans_of_its_own_units(oracle):
    meta, arr, fasta = G.load("c1_se36")
    gref = B.RefSeq(B.make_params(**meta["kw"])).Run_ConvertBinseq(fasta_path=fasta).CreateIndex()
    al = _load_batch(meta, gref)
    try:
        al.set_all_hits(POOL)
        al.Do_Batch()
        spans, pool = al.all_hits()
        full = [B.all_hits_lists(spans[i], pool) for i in range(len(spans))]
        al.run_range(100, 200, sync=True)
        s2, p2 = al.all_hits(200)
        need, _ = check_spans(al, s2, p2)
        assert need == int((spans["n"][100:300, 0].astype(np.int64) * 2).sum())
        assert [B.all_hits_lists(s2[i], p2) for i in range(200)] == full[100:300]
    finally:
        al.close()
        gref.close()


@pytest.mark.parametrize("name", ["c5_trim_pe150", "c1_se36"])
def test_exact_mode_lists_equal_the_goldens_for_every_unit(name):
    """bsx_batch_set_leak_exact with a pool: the reference's single-threaded lists for EVERY unit, the call-order dependent ones included"""
    meta, arr, fasta = G.load(name)
    kw, kind = meta["kw"], meta["kind"]
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_path=fasta).CreateIndex()
    al = _load_batch(meta, gref).set_leak_exact()
    try:
        res, spans, pool = _run_twice(al)
        check_spans(al, spans, pool)
        emitting = 0
        for i, e in enumerate(meta["expected"]):
            want = tuple(golden_lists(e, kind, kw["v"] + 1))
            assert B.all_hits_lists(spans[i], pool) == want, (name, i)
            emitting += any(want)
        assert emitting == EMITTING[name][0]
        assert check_picks(kind, res, spans, pool, kw.get("S", 0)) == emitting
    finally:
        al.close()
        gref.close()
