"""The HIP path on the directed boundary reads of tests/test_oracle_boundaries.py (bsx_testdata.boundary_*): reads at letters 0, 1, 2, 15..48
from both ends of every chromosome, sticking out of a chromosome (the outside letters random, or exactly what the packed array holds there, so
that the bounds test alone rejects the candidate), abutting N runs, inside 29- and 30-letter islands, of every length from the seed size to 144,
with 0, 1, v and v + 1 placed mismatches, pairs with inserts at and around -m and -x, RRBS reads from every site.  Needs an MI355X.

The oracle is pinned to the real reference on exactly these reads (tests/golden/boundaries_vs_reference.json.gz); here the same reads go
through the C ABI with debug on and EVERY unit of every case is compared with the oracle, filtered reads included:
  single-end: filtered flag, lengths, max_snp, seedseg, planner arrays, all class counts, every hit list of every class and orientation, the pick;
  pairs:      the same per mate, paired, n_pairs, every pair list, the pick fields, unpaired_out;
  the four work counters where they are on; the index (offsets, forward counts, entries) first.
Routes (PLAN below): the default; work counters off, which is where the main kernel takes its context prefilter (wave_scan_range<.., CTX>: the 32
reference nt on either side of the seed, stored by k_context — at a chromosome end those are pad letters, the neighbour or the margin, at a read
end the flank words are masked out); the same without a context table; the heavy pipeline forced (its own lane-mask bounds test, k_hscan /
k_hscan_same / k_hscan_shared with their per-length loops) with and without counters; exact mode against the oracle in call order; all hits.
Where two routes must give the same records their result bytes are compared too, so that a discrepancy names the route.

What the file is for: it fails when k_context stores 0 for its word j == 0, when hit_coords says >= for >, and when the 65-96 nt loop of
k_hscan_shared drops its third word; the drawn reads of tests/test_gpu_parity.py pass with the second of these."""
import pytest

import numpy as np

import bsmap_amd as B
import test_oracle_boundaries as TB

pytestmark = pytest.mark.gpu

CASES = TB.all_cases()
SE = ["test_se[%s]" % TB._id(kw) for kw in TB.SE_CASES]
PE = ["test_pe[%s]" % TB._id(c["kw"]) for c in TB.PE_CASES]
RR = ["test_rrbs[%s]" % TB._id(kw) for kw in TB.RRBS_CASES]
POOL = 1 << 22   # all-hits pool, words


def _plan():
    """(case, route) in case order: the reference and the oracle's records of a case are built once and serve all its routes"""
    routes = {n: ["default", "counters_off"] for n in CASES}
    for n in SE + PE:
        if CASES[n][1]["kw"]["I"] <= 4:
            routes[n].append("no_context")
    for n in (SE[3], SE[6], PE[4]):          # -s 9: candidate lists of 48 and more exist on this genome
        routes[n] += ["heavy", "heavy_counters_off"]
    routes[SE[6]].append("heavy_same0")
    for n in RR:
        routes[n] += ["heavy_same1", "heavy_same1_counters_off", "heavy_same2"]
    routes[RR[0]].append("heavy_same2_counters_off")
    for n in (SE[0], SE[1], SE[3], SE[4], SE[6], PE[0], PE[2], PE[4]):
        routes[n].append("exact")
    for n in (SE[0], PE[0]):                 # exact mode on top of the context prefilter
        routes[n].append("exact_counters_off")
    for n in (SE[2], SE[3], SE[6], PE[4]):   # -r 1 and units with several equal-best placements (the short reads of class D, the mates of 26..29 letters)
        routes[n].append("all_hits")
    return [(n, r) for n in CASES for r in routes[n]]


PLAN = _plan()


# ---- what the oracle says about a unit, as plain data ---------------------------------------------------------------------------------

def _exp_read(o, hits, nclass):
    d = dict(filtered=bool(o.filtered), len=o.len, raw_len=o.raw_len)
    if o.filtered:
        return d
    n = o.seedseg_num
    d.update(max_snp=o.read_max_snp_num, seedseg=n,
             plan=[list(o.seed_start_array)[:n], list(o.seedindex)[:n]] if o.flag_chain else None,
             cplan=[list(o.cseed_start_array)[:n], list(o.cseedindex)[:n]] if o.cflag_chain else None,
             n_hit=list(o.n_hit)[:nclass], n_chit=list(o.n_chit)[:nclass],
             lists=[[hits(orient, w, (o.n_chit if orient else o.n_hit)[w]) for orient in (0, 1)] for w in range(nclass)],
             pick=(o.n_best, o.best_class, o.chr, o.loc, o.chain) if o.n_best > 0 else (0, -1))
    return d


def _expected(oracle, oref, kind, kw, reads, leak_mode):
    """(records, work counters) of the oracle for every unit of a case"""
    nclass = kw["v"] + 1
    al = oracle.OracleAligner(oref, leak_mode=leak_mode)
    out = []
    for i, r in enumerate(reads):
        if kind == "pe":
            o = al.pe(i, r["seq1"], r["seq2"], r["qual1"], r["qual2"])
            up = bool(o.tmp == 1 or o.paired == 0)
            pk = o.pick
            d = dict(paired=o.paired, n_pairs=list(o.n_pairs)[:2 * nclass - 1], unpaired_out=up,
                     a=_exp_read(o.a, lambda orient, w, n: al.pe_hits(0, orient, w, n), nclass),
                     b=_exp_read(o.b, lambda orient, w, n: al.pe_hits(1, orient, w, n), nclass),
                     pairs=[al.pe_pairs(w, o.n_pairs[w]) for w in range(2 * nclass - 1)],
                     pick=None if up else (pk.chain, pk.na, pk.nb, pk.insert, pk.a.chr, pk.a.loc, pk.b.chr, pk.b.loc, o.pair_class, o.pair_n))
            for m in "ab":
                d[m].pop("plan", None), d[m].pop("cplan", None)   # (the pairs' comparison is the records, lists and picks)
                if not up:
                    d[m].pop("pick", None)                       # a reported pair: the mates' own picks are not output
            out.append(d)
        else:
            out.append(_exp_read(al.se(i, r["seq"], r["qual"]), al.se_hits, nclass))
    cnt = al.counters()
    al.free()
    return out, cnt


# ---- the same of the device batch ------------------------------------------------------------------------------------------------------

def _got_read(bt, i, mate, h, cc, nclass, e):
    d = dict(filtered=bool(h["flags"] & B.F_FILTERED), len=int(h["len"]), raw_len=int(h["raw_len"]))
    if d["filtered"] or e["filtered"]:
        return d
    n = int(h["seedseg"])
    d.update(max_snp=int(h["max_snp"]), seedseg=n, n_hit=[int(x) for x in cc["n_hit"][:nclass]], n_chit=[int(x) for x in cc["n_chit"][:nclass]])
    if "plan" in e:
        st, od = bt.debug_plan(i, mate)
        d["plan"] = [[int(x) for x in st[0][:n]], [int(x) for x in od[0][:n]]] if e["plan"] is not None else None
        d["cplan"] = [[int(x) for x in st[1][:n]], [int(x) for x in od[1][:n]]] if e["cplan"] is not None else None
    # (a list whose count is 0 on both sides is empty on both sides: bsx_batch_debug_hits returns the first `count` entries)
    d["lists"] = [[bt.debug_hits(i, mate, orient, w) if (d["n_chit"] if orient else d["n_hit"])[w] or (e["n_chit"] if orient else e["n_hit"])[w] else []
                   for orient in (0, 1)] for w in range(nclass)]
    if "pick" in e:
        d["pick"] = (int(h["n_best"]), int(h["best_class"]), int(h["chr"]), int(h["loc"]), int(h["flags"] >> 1) & 1) if h["n_best"] > 0 else (0, int(h["best_class"]))
    return d


def _diff(e, g):
    if isinstance(e, dict):
        for k in e:
            if k not in g or e[k] != g[k]:
                return "%s: %s" % (k, _diff(e[k], g.get(k)) if isinstance(e[k], dict) and isinstance(g.get(k), dict) else "oracle %r, device %r" % (e[k], g.get(k)))
        return "device has %s more" % sorted(set(g) - set(e))
    return "oracle %r, device %r" % (e, g)


def _compare(kind, kw, reads, exp, bt, res, route):
    """every unit of the batch against the oracle's records"""
    nclass = kw["v"] + 1
    for i, (r, e) in enumerate(zip(reads, exp)):
        if kind == "pe":
            out, ca, cb, npairs = res
            g = out[i]
            up = bool(g["unpaired_out"])
            d = dict(paired=int(g["paired"]), n_pairs=[int(x) for x in npairs[i][:2 * nclass - 1]], unpaired_out=up,
                     a=_got_read(bt, i, 0, g["a"], ca[i], nclass, e["a"]), b=_got_read(bt, i, 1, g["b"], cb[i], nclass, e["b"]),
                     pairs=[bt.debug_pairs(i, w) if npairs[i][w] or e["n_pairs"][w] else [] for w in range(2 * nclass - 1)],
                     pick=None if up else (int(g["chain"]), int(g["na"]), int(g["nb"]), int(g["insert"]), int(g["a_chr"]), int(g["a_loc"]), int(g["b_chr"]),
                                           int(g["b_loc"]), int(g["pair_class"]), int(g["n_pairs"])))
        else:
            hits, cc = res
            d = _got_read(bt, i, 0, hits[i], cc[i], nclass, e)
        assert d == e, "route %s, unit %d (%s): %s" % (route, i, r["name"], _diff(e, d))


class _Case:
    """one case with its reference on the device and in the oracle; the records the oracle gives its reads, by leak mode"""

    def __init__(self, name, d, oracle):
        self.name, self.oracle = name, oracle
        self.kind, case = CASES[name]
        self.kw, self.g, self.fa, self.reads = TB.case_inputs(self.kind, case, d)
        self.oref = oracle.OracleRef(oracle.make_params(**self.kw), fasta_path=self.fa)
        self.gref = B.RefSeq(B.make_params(**self.kw)).Run_ConvertBinseq(fasta_path=self.fa).CreateIndex()
        self.exp, self.bytes = {}, {}

    def expected(self, leak_mode=0):
        if leak_mode not in self.exp:
            self.exp[leak_mode] = _expected(self.oracle, self.oref, self.kind, self.kw, self.reads, leak_mode)
        return self.exp[leak_mode]

    def batch(self, gref=None, debug=True):
        gref = gref or self.gref
        rd = self.reads
        if self.kind == "pe":
            bt = B.PairAlign(gref, len(rd), debug=debug)
            return bt, lambda: bt.ImportBatchReads([r["seq1"] for r in rd], [r["seq2"] for r in rd], [r["qual1"] for r in rd], [r["qual2"] for r in rd])
        bt = B.SingleAlign(gref, len(rd), debug=debug)
        return bt, lambda: bt.ImportBatchReads([r["seq"] for r in rd], [r["qual"] for r in rd])

    def run(self, route, counters=True, leak_mode=0, gref=None, expect_heavy=False, same_as=None):
        """one debug batch over the case's reads: every unit against the oracle, the work counters where they are on, heavy units where the
        route forces them, and the result bytes against those of the route that must give the same records"""
        if same_as is not None and same_as not in self.bytes:
            self.run(same_as, counters=same_as == "default")
        bt, upload = self.batch(gref)
        try:
            bt.set_work_counters(counters)
            if leak_mode:
                bt.set_leak_exact()
            upload().Do_Batch()
            res = bt.results()
            exp, cnt = self.expected(leak_mode)
            _compare(self.kind, self.kw, self.reads, exp, bt, res, route)
            c = bt.counters()
            if counters:
                assert [int(x) for x in c[:4]] == cnt, (route, [int(x) for x in c[:4]], cnt)
            if self.kind != "pe" and route == "default":
                assert int(c[4]) == len(self.reads)
            if expect_heavy:
                assert bt.heavy_units() > 0, route
            else:
                assert bt.heavy_units() == 0, route
            self.bytes[route] = tuple(a.tobytes() for a in res)
            if same_as is not None:
                assert self.bytes[route] == self.bytes[same_as], "routes %s and %s give different result bytes" % (route, same_as)
        finally:
            bt.close()

    def close(self):
        self.gref.close()
        self.oref.free()


_live = []


@pytest.fixture(scope="module")
def cases(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("boundaries")

    def get(name):
        if not _live or _live[0].name != name:
            while _live:
                _live.pop().close()
            _live.append(_Case(name, d, oracle))
        return _live[0]
    yield get
    while _live:
        _live.pop().close()


def _forced_heavy(c, route, monkeypatch, same, counters):
    if same is not None:
        monkeypatch.setenv("BSX_SAME", same)   # read when the batch is created
    base = "default" if counters else "counters_off"
    if base not in c.bytes:
        c.run(base, counters=counters)   # (the route to compare with, before the threshold is forced)
    B.lib().bsx_set_heavy_threshold(2 if c.kind == "rrbs" else 48)
    try:
        c.run(route, counters=counters, expect_heavy=True, same_as=base)
    finally:
        B.lib().bsx_set_heavy_threshold(0)


def _all_hits(c):
    """a production-mode batch with an all-hits pool: the spans of every multi-hit unit are the oracle's lists of its best class"""
    exp, _ = c.expected(0)
    bt, upload = c.batch(debug=False)
    try:
        bt.set_all_hits(POOL)
        upload().Do_Batch()
        spans, pool = bt.all_hits()
        need, dropped = bt.all_hits_need()
        assert dropped == 0
        n_multi = 0
        for i, e in enumerate(exp):
            la, lb, lp = B.all_hits_lists(spans[i], pool)
            if c.kind == "pe":
                if not e["unpaired_out"]:
                    w, n = e["pick"][8], e["pick"][9]
                    want = ([], [], e["pairs"][w] if n >= 2 else [])
                else:
                    want = tuple([] if m["filtered"] or m["pick"][0] < 2 else m["lists"][m["pick"][1]][0] + m["lists"][m["pick"][1]][1] for m in (e["a"], e["b"])) + ([],)
            else:
                want = ([] if e["filtered"] or e["pick"][0] < 2 else e["lists"][e["pick"][1]][0] + e["lists"][e["pick"][1]][1], [], [])
            assert (la, lb, lp) == want, "all hits, unit %d (%s)" % (i, c.reads[i]["name"])
            n_multi += any(want)
        assert n_multi > 0, "no multi-hit unit in the case"
    finally:
        bt.close()


@pytest.mark.parametrize("name,route", PLAN, ids=["%s-%s" % (n.split("[")[1][:-1], r) for n, r in PLAN])
def test_boundary_reads(name, route, cases, monkeypatch):
    c = cases(name)
    kw = c.kw
    wgbs_ctx = c.kind != "rrbs" and kw["I"] <= 4
    if route == "default":
        g, o = c.gref, c.oref
        if c.kind != "rrbs":
            assert g.packed_on_device                                   # the FASTA text exceeds 64 KB: the device packer built the words
        assert (g.context_bytes > 0) == wgbs_ctx, g.context_bytes        # the prefilter's table exists for WGBS with -I <= 4
        a, s, r = g.info()
        assert np.array_equal(a, o.anchor()) and np.array_equal(s, o.chr_size()) and np.array_equal(r, o.rc_offset()) and g.names() == o.names()
        assert np.array_equal(g.blocks(), o.blocks())
        f, cw = g.words()
        assert np.array_equal(f[400:-400], o.refcat()[400:-400]) and np.array_equal(cw[400:-400], o.crefcat()[400:-400])
        off, nf, ent = g.index()
        assert np.array_equal(off, o.bucket_off())
        if c.kind == "rrbs":
            assert np.array_equal(np.asarray(ent).reshape(-1, 2), o.rrbs_entries())
            for ci in range(g.n_chr):
                assert np.array_equal(g.sites(ci), o.sites(ci))
        else:
            assert np.array_equal(nf, o.bucket_nfwd()) and np.array_equal(ent, o.entries())
        c.run("default")
    elif route == "counters_off":
        c.run("counters_off", counters=False)
    elif route == "no_context":
        g2 = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_path=c.fa).CreateIndex(context=0)
        try:
            assert g2.context_bytes == 0 and c.gref.context_bytes > 0
            c.run("no_context", counters=False, gref=g2, same_as="counters_off")
        finally:
            g2.close()
    elif route.startswith("heavy"):
        same = {"heavy_same0": "0", "heavy_same1": "1", "heavy_same2": "2"}.get(route.replace("_counters_off", ""))
        _forced_heavy(c, route, monkeypatch, same, counters=not route.endswith("counters_off"))
    elif route in ("exact", "exact_counters_off"):
        c.run(route, counters=route == "exact", leak_mode=1)
    elif route == "all_hits":
        _all_hits(c)
    else:
        raise AssertionError(route)
