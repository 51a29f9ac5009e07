"""One batch through every member it creates lazily, replaces or drops (bsx_api.hip: each is an owner — DevBuf, DevEvent — of the batch handle), in ONE
process and on ONE handle: the all-hits pool attached, resized and detached; the debug arrays and the per-unit slabs; the exact mode's arrays with a
history and an initial state, both replaced and dropped again; the read buffers regrown by an upload longer than their capacity; then the handle destroyed and
a second one created.  Records and class counts equal the oracle's after every run.  What each feature computes is held elsewhere (test_gpu_all_hits.py,
test_gpu_leak_exact.py, test_gpu_parity.py, each on handles of their own); this test holds the transitions between them."""
import numpy as np
import pytest

import bsmap_amd as B
import bsx_testdata as td

pytestmark = pytest.mark.gpu

N, NZ, NH = 4096, 512, 64   # units of the batch; reads in front of them in the exact mode's stream: those that only leave a state, those attached as history
TAIL = "ACGT" * 15          # appended to 144-nt reads: 204 letters, of which both sides keep -L 144 — 4 096 of them are longer than the buffers of a 4 096-unit batch


def check_se(ores, hits, cc, nclass):
    ok = ores["filtered"] == 0
    assert np.array_equal(ores["n_hit"][ok][:, :nclass], cc["n_hit"][ok][:, :nclass]) and np.array_equal(ores["n_chit"][ok][:, :nclass], cc["n_chit"][ok][:, :nclass])
    has = ok & (ores["n_best"] > 0)
    assert has.sum() > len(has) // 2
    for f in ("chr", "loc", "best_class"):
        assert np.array_equal(ores[f][has], hits[f][has]), f


def check_pe(ores, res, nclass):
    out, ca, cb, npairs = res
    assert np.array_equal(ores["paired"], out["paired"]) and np.array_equal(ores["n_pairs"][:, :2 * nclass - 1], npairs[:, :2 * nclass - 1])
    assert np.array_equal(ores["a"]["n_hit"][:, :nclass], ca["n_hit"][:, :nclass]) and np.array_equal(ores["b"]["n_chit"][:, :nclass], cb["n_chit"][:, :nclass])
    pr = (ores["tmp"] == 0) & (ores["paired"] > 0)
    assert pr.sum() > len(pr) // 2
    for f in ("a_chr", "a_loc", "b_chr", "b_loc", "insert"):
        assert np.array_equal(ores["pick"][f][pr], out[f][pr]), f


@pytest.mark.parametrize("pe", [False, True], ids=["se", "pe"])
def test_one_handle_through_every_lazy_member(pe, oracle):
    g = td.make_genome(seed=3, chr_lens=(120_000, 40_000), gc=0.5)   # (the genome of smoke())
    fasta = td.fasta_text(g)
    kw = dict(s=16, v=6, I=4, S=1, r=1, m=28, x=500, pairend=1) if pe else dict(s=16, v=4, I=4, S=1, r=1)
    nclass = kw["v"] + 1
    oref = oracle.OracleRef(oracle.make_params(**kw), fasta_text=fasta)
    gref = B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_text=fasta).CreateIndex()
    rng = np.random.default_rng(17)
    total = NZ + NH + N
    # a third of the reads end where (len - I + 1) % s == 0: those take their plan's start from the reads in front of them in exact mode
    cut = lambda L: [L if k else int(x) for k, x in zip(rng.integers(0, 3, total), rng.choice([L - 13, L - 29, L - 45], total))]
    if pe:
        pairs = td.make_pe_reads(g, total, 144, seed=6)
        streams = [[p[key][:l] for p, l in zip(pairs, cut(144))] for key in ("seq1", "seq2")]
        long_ = [[p[key] + TAIL for p in pairs[:N]] for key in ("seq1", "seq2")]
    else:
        reads = td.make_se_reads(g, total, 144, seed=5)
        streams = [[r["seq"][:l] for r, l in zip(reads, cut(144))]]
        long_ = [[r["seq"] + TAIL for r in reads[:N]]]

    def expected(seqs, first_index=0, leak_mode=0):
        packed = [x for s in seqs for x in oracle.pack_reads(s)]
        if pe:
            return oracle.pe_batch(oref, *packed, first_index=first_index, threads=8, leak_mode=leak_mode)[0]
        return oracle.se_batch(oref, *packed, first_index=first_index, threads=8, leak_mode=leak_mode)[0]

    def run(al, seqs, first_index=0):
        al.ImportBatchReads(*seqs, first_index=first_index).Do_Batch()
        return al.results()

    def check(ores, res):
        check_pe(ores, res, nclass) if pe else check_se(ores, res[0], res[1], nclass)

    units = [s[NZ + NH:] for s in streams]
    e_plain = expected(units, first_index=NZ + NH)
    e_exact = expected(streams, leak_mode=1)
    e_long = expected(long_)
    part = lambda e, lo, hi: e[lo:hi]   # (the oracle's records are one array)
    Align = B.PairAlign if pe else B.SingleAlign
    al = Align(gref, N)
    try:
        assert sum(len(x) for x in long_[0]) + 256 > N * 160 + 256   # (the upload at the end does not fit the buffers the handle starts with)
        # the all-hits pool: attached, filled, replaced by a larger one, filled, dropped
        al.set_all_hits(1 << 18)
        first = run(al, units, NZ + NH)
        check(e_plain, first)
        need, dropped = al.all_hits_need()
        spans, pool = al.all_hits()
        assert dropped == 0 and need == len(pool) < (1 << 18) and spans.shape == (N, 3)
        al.set_all_hits(need + 4096)
        check(e_plain, run(al, units, NZ + NH))
        assert al.all_hits_need() == (need, 0) and len(al.all_hits()[1]) == need
        al.set_all_hits(0)
        with pytest.raises(B.BsxError):
            al.all_hits_need()
        # the debug mode: a slab per unit, the plans kept
        al.set_debug(1)
        check(e_plain, run(al, units, NZ + NH))
        oa = oracle.OracleAligner(oref, 0)
        for i in range(16):
            if pe:
                o = oa.pe(NZ + NH + i, units[0][i], units[1][i])
                for mate, om in enumerate((o.a, o.b)):
                    al.debug_plan(i, mate)
                    for w in range(nclass if not om.filtered else 0):
                        for orient in (0, 1):
                            assert al.debug_hits(i, mate, orient, w) == oa.pe_hits(mate, orient, w, (om.n_chit if orient else om.n_hit)[w]), (i, mate, w, orient)
            else:
                o = oa.se(NZ + NH + i, units[0][i])
                st, od = al.debug_plan(i)
                n = o.seedseg_num
                if not o.filtered and o.flag_chain:
                    assert list(st[0][:n]) == list(o.seed_start_array)[:n] and list(od[0][:n]) == list(o.seedindex)[:n], i
                for w in range(nclass if not o.filtered else 0):
                    for orient in (0, 1):
                        assert al.debug_hits(i, 0, orient, w) == oa.se_hits(orient, w, (o.n_chit if orient else o.n_hit)[w]), (i, w, orient)
        oa.free()
        al.set_debug(0)
        check(e_plain, run(al, units, NZ + NH))
        # the exact mode: the first reads of the stream only leave their state; the units start from it, with the reads in between as history
        al.set_leak_exact(True)
        check(part(e_exact, 0, NZ), run(al, [s[:NZ] for s in streams]))
        st0 = al.get_leak_state()
        al.set_history(*[x for s in streams for x in (s[NZ:NZ + NH], None)])
        al.set_leak_state(st0)
        check(part(e_exact, NZ + NH, total), run(al, units, NZ + NH))
        st_end = al.get_leak_state()
        # ... and the same stream cut elsewhere: from no state and no history, then from that state and another history
        al.set_history(*[x for s in streams for x in ([], None)])
        al.set_leak_state(None)
        check(part(e_exact, 0, N), run(al, [s[:N] for s in streams]))
        st1 = al.get_leak_state()
        al.set_history(*[x for s in streams for x in (s[N - NH:N], None)])
        al.set_leak_state(st1)
        check(part(e_exact, N, total), run(al, [s[N:] for s in streams], N))
        assert al.get_leak_state().tobytes() == st_end.tobytes() and st_end.any()
        al.set_leak_exact(False)
        al.set_history(*[x for s in streams for x in ([], None)])
        # reads longer than the buffers: both are replaced
        check(e_long, run(al, long_))
        check(e_plain, run(al, units, NZ + NH))
    finally:
        al.close()
    again = Align(gref, N)
    try:
        again.set_all_hits(1 << 18)
        second = run(again, units, NZ + NH)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
        assert again.all_hits_need() == (need, 0)
    finally:
        again.close()
        gref.close(); oref.free()
