"""BASELINE-sized checks (hg38-sized synthetic genome, 3.09 Gbp, 1.48 G index entries; the bench workload).
Parity at this size:
  * the seed index itself: the oracle packs and indexes the genome TEXT pulled back from the device (its restatement of
    dbseq.cpp:308-481, one thread, minutes) and every packed word, bucket offset, forward count and entry of the GPU-built
    index (k_enumerate -> radix sort -> k_boundaries, 1.476 G entries) must equal it — once per session for WGBS (-s 16 -I 4,
    all WGBS configs share it), and for the RRBS {tag, loc} index of C4;
  * WHOLE batches (131 072 units of C2 / C3, 65 536 of C2 -n 1 / C4 / C5) re-aligned by the oracle's batch driver on the host
    cores against the ORACLE-BUILT reference + index: every record field and the four work counters; C5 also in exact mode
    against the oracle's `-p 1` state; a summary goes to gpurun_out/validate/r04_validate_<cfg>.json (copied into profiles/);
  * bench steps (test_blocks_of_a_bench_sized_batch_equal_the_oracle, test_bench_step_equals_the_oracle): one step of bench.py's own size, pools and
    reads per mode (C2 / C3 / C4 / C5), blocks of it and deferred units from every round of the heavy pipeline re-aligned by the oracle (wholebatch.py);
  * idempotence: the same batch twice gives byte-identical records and counters;
  * partition invariance: aligning in two halves equals aligning the whole batch;
  * path invariance: results do not depend on which units go through the heavy pipeline (default threshold vs none);
  * geometry: reads were sampled as 50..480 nt fragments; reported pairs are same-chromosome, insert in range, >95 % unique;
  * counter closure: units processed == units submitted."""
import hashlib
import time

import numpy as np
import pytest

import bsmap_amd as B

pytestmark = pytest.mark.gpu

HG38 = [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422,
        135086622, 133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167,
        46709983, 50818468, 156040895, 57227415]
KW = dict(s=16, v=6, I=4, m=28, x=500, S=1, r=1, pairend=1)
N = 131072


@pytest.fixture(scope="module")
def big():
    ref = B.RefSeq(B.make_params(**KW)).synthetic(HG38, seed=38).CreateIndex()
    pa = B.PairAlign(ref, N)
    pa.synth_reads(N, 144, seed=11)
    pa.Do_Batch()
    out, ca, cb, npairs = pa.results()
    cnt = pa.counters().copy()
    HEAVY["c3"] = int(pa.heavy_units())   # of THIS run (later tests run parts of the batch again)
    yield ref, pa, out.copy(), ca.copy(), cb.copy(), npairs.copy(), cnt
    pa.close()
    ref.close()


HEAVY = {}


def _genome_text(ref):
    parts = []
    for c, nm in enumerate(ref.names()):
        parts += [np.frombuffer(f">{nm}\n".encode(), np.uint8), ref.synth_bytes(c), np.frombuffer(b"\n", np.uint8)]
    return np.concatenate(parts).tobytes()


class _OracleWgbs:
    """The oracle's OWN reference + WGBS index of the hg38-sized genome, built once per session from the genome text (-s 16 -I 4:
    what every WGBS config here uses), and the proof that a GPU-built reference equals it."""

    def __init__(self, oracle):
        self.oracle, self.base, self.info = oracle, None, None

    def _build(self, ref):
        text = _genome_text(ref)
        t0 = time.time()
        self.base = self.oracle.OracleRef(self.oracle.make_params(**KW), fasta_text=text)
        self.build_s = time.time() - t0

    def check(self, ref, name):
        """every word / offset / count / entry of the GPU-built reference `ref` against the oracle's build"""
        if self.base is None:
            self._build(ref)
        o = self.base
        f, c = ref.words()
        assert np.array_equal(f, o.refcat()) and np.array_equal(c, o.crefcat())
        a, s, r = ref.info()
        assert np.array_equal(a, o.anchor()) and np.array_equal(s, o.chr_size()) and np.array_equal(r, o.rc_offset())
        del f, c
        off, nf, ent = ref.index()
        assert len(ent) == o.r.n_entries == ref.n_entries
        assert np.array_equal(off, o.bucket_off()), "bucket offsets"
        assert np.array_equal(nf, o.bucket_nfwd()), "forward counts"
        assert np.array_equal(ent, o.entries()), "entries"
        if self.info is None:
            sizes = np.diff(off.astype(np.int64))
            self.info = dict(entries=int(len(ent)), buckets=int(len(nf)), non_empty_buckets=int((sizes > 0).sum()), largest_bucket=int(sizes.max()),
                             entries_sha256=hashlib.sha256(ent.tobytes()).hexdigest(), bucket_off_sha256=hashlib.sha256(off.tobytes()).hexdigest(),
                             oracle_build_s=round(self.build_s, 1), checked=[])
        self.info["checked"].append(name)
        import wholebatch as W
        W.record("index", self.info)

    def ref_for(self, kw):
        """the oracle-built arrays under another config's parameters (same -s / -I)"""
        o = self.base
        return self.oracle.OracleRef.wrap(self.oracle.make_params(**kw), o.refcat(), o.crefcat(), o.anchor(), o.chr_size(), o.rc_offset(),
                                          o.bucket_off(), o.bucket_nfwd(), o.entries())


@pytest.fixture(scope="session")
def oracle_wgbs(oracle):
    w = _OracleWgbs(oracle)
    yield w
    if w.base is not None:
        w.base.free()


def test_gpu_built_index_equals_the_oracles_own_build(big, oracle_wgbs):
    """RefSeq::CreateIndex at BASELINE size (dbseq.cpp:308-481): 1.476 G entries through 64-bit enumeration, 32-bit keys and a
    radix sort on the device against the oracle's count / prefix / fill from the genome text"""
    ref = big[0]
    oracle_wgbs.check(ref, "c3")
    assert oracle_wgbs.info["entries"] > 1_400_000_000


def test_sizes_and_closure(big):
    ref, pa, out, ca, cb, npairs, cnt = big
    assert ref.n_entries > 1_400_000_000 and ref.n_words > 190_000_000
    assert int(cnt[4]) == N and pa.heavy_units() > N // 200
    assert (out["unpaired_out"] == 0).mean() > 0.99


def test_idempotent_and_partition_invariant(big):
    ref, pa, out, ca, cb, npairs, cnt = big
    pa.reset_counters()
    pa.Do_Batch()
    out2, ca2, cb2, np2 = pa.results()
    assert out2.tobytes() == out.tobytes() and ca2.tobytes() == ca.tobytes() and np2.tobytes() == npairs.tobytes()
    assert np.array_equal(pa.counters()[:7], cnt[:7])
    pa.run_range(N // 2, N // 2, sync=True)
    pa.run_range(0, N // 2, sync=True)
    out3, ca3, cb3, np3 = pa.results()
    assert out3.tobytes() == out.tobytes() and cb3.tobytes() == cb.tobytes()


def test_records_do_not_depend_on_the_work_counters(big):
    """with the work counters off (bsx_batch_set_work_counters: the scan kernels skip the early-out classification, the control kernel its
    count-only walks — what the command line and bench.py's timed region run) every record is byte-identical and the aligned counts agree"""
    ref, pa, out, ca, cb, npairs, cnt = big
    pa.set_work_counters(False)
    try:
        pa.reset_counters()
        pa.Do_Batch()
        out2, ca2, cb2, np2 = pa.results()
        c2 = pa.counters()
    finally:
        pa.set_work_counters(True)
    assert out2.tobytes() == out.tobytes() and ca2.tobytes() == ca.tobytes() and cb2.tobytes() == cb.tobytes() and np2.tobytes() == npairs.tobytes()
    assert np.array_equal(c2[4:7], cnt[4:7]) and int(c2[2]) < int(cnt[2])   # (sum_w is what is no longer counted)
    assert pa.heavy_units() == HEAVY["c3"]


def test_heavy_path_invariance(big):
    ref, pa, out, ca, cb, npairs, cnt = big
    # 4096 units through the one-wave path only (threshold so high that nothing is deferred)
    B.lib().bsx_set_heavy_threshold(1 << 30)
    try:
        pa.reset_counters()
        pa.run_range(0, 2048, sync=True)
        assert pa.heavy_units() == 0
        o2, a2, b2, n2 = pa.results()
    finally:
        B.lib().bsx_set_heavy_threshold(0)
    assert o2[:2048].tobytes() == out[:2048].tobytes() and a2[:2048].tobytes() == ca[:2048].tobytes() and n2[:2048].tobytes() == npairs[:2048].tobytes()


def test_whole_batch_equals_oracle_c3(big, oracle, oracle_wgbs):
    """every unit of the batch re-aligned by the oracle's batch driver against the ORACLE's own reference + index (shown equal
    to the device's in the test above): every record field and the four work counters (the roofline numerator)"""
    import wholebatch as W
    ref, pa, out, ca, cb, npairs, cnt = big
    if oracle_wgbs.base is None:
        oracle_wgbs.check(ref, "c3")
    oref = oracle_wgbs.ref_for(KW)
    ores, ocnt, t_cpu = W.run_oracle(oracle, oref, pa, True, False, N)
    bad, info = W.compare_pe(ores, out, ca, cb, npairs, KW["v"] + 1)
    W.record("c3", dict(info, units=N, oracle_s=round(t_cpu, 1), counters_gpu=[int(x) for x in cnt[:4]], counters_oracle=ocnt, mismatching_fields=bad,
                        options=KW, heavy_units=HEAVY["c3"], reference="oracle-built from the genome text"))
    assert not bad, bad
    assert [int(x) for x in cnt[:4]] == ocnt


def test_blocks_of_a_bench_sized_batch_equal_the_oracle(big, oracle, oracle_wgbs):
    """bench.py's own step — 2^22 pairs, read seed 3, unit ids from 0, the pools the bench gives it, work counters off as in the timed region — run as
    ONE batch (its deferred units are grouped as in the bench: 37 K of them), and 32 blocks of 4 096 consecutive units spread over the batch (2^17 units)
    re-aligned by the oracle against its own reference + index: every record field.  (Round 4 validated the 2^20-pair bench batch with a tool outside
    the suite, profiles/r04h_validate_full_c3.json.)"""
    import wholebatch as W
    ref = big[0]
    if oracle_wgbs.base is None:
        oracle_wgbs.check(ref, "c3")
    oref = oracle_wgbs.ref_for(KW)
    M, NB, _, limits = W.bench_mode("pe")
    assert M["kw"] == KW and NB == 1 << 22
    BLK, NBLK = 4096, 32
    pa = W.bench_batch(ref, "pe", NB)
    try:
        pa.synth_reads(NB, M["L"], seed=3, kind=M["kind"])
        # the deferred units carry 97 % of the step's candidates: the comparison has to hold a good number of them — those that fall into the blocks,
        # and 256 more taken evenly from the deferred list, each re-aligned alone
        bad_all, info = W.bench_step_blocks(oracle, oref, pa, "pe", 0, n_blocks=NBLK, blk=BLK)
    finally:
        pa.close()
    W.record("bench_step_c3", info)
    heavy = info["heavy_units"]
    assert info["deferred_in_blocks"] >= 1000 and info["deferred_alone"] >= 200, info
    assert info["pool_sizes"] == list(limits), info
    assert heavy > NB // 200 and info["paired_out"] > 0.95 * BLK * NBLK
    assert not bad_all, bad_all


def test_pair_geometry(big):
    """the sampler draws fragments of 50..480 nt from one chromosome: reported pairs must respect that geometry"""
    ref, pa, out, ca, cb, npairs, cnt = big
    pr = out["unpaired_out"] == 0
    # both mates on the same chromosome copy, insert within [50, 480] as sampled, mates facing each other
    assert np.array_equal(out["a_chr"][pr], out["b_chr"][pr])
    ins = out["insert"][pr]
    assert ins.min() >= 28 and ins.max() <= 500 and 250 < np.median(ins) < 350
    uniq = pr & (out["n_pairs"] == 1)
    assert uniq.mean() > 0.95


def test_two_batches_in_flight(big):
    """two device batches driven by two host threads at the same time (what bench.py and the command-line driver do):
    same records as the batch that ran alone"""
    import threading
    ref, pa, out, ca, cb, npairs, cnt = big
    others = [B.PairAlign(ref, N) for _ in range(2)]
    res = [None, None]
    try:
        for o in others:
            o.synth_reads(N, 144, seed=11)

        def work(j):
            for _ in range(2):
                others[j].Do_Batch()
            res[j] = tuple(x.copy() for x in others[j].results())

        th = [threading.Thread(target=work, args=(j,)) for j in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for j in range(2):
            o2, a2, b2, n2 = res[j]
            assert o2.tobytes() == out.tobytes() and a2.tobytes() == ca.tobytes() and b2.tobytes() == cb.tobytes() and n2.tobytes() == npairs.tobytes()
    finally:
        for o in others:
            o.close()


# ---- the other BASELINE configurations at the same scale --------------------------------------------------------------
ADAPTER = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"
OTHER = {
    # C2: 1x100 WGBS, -v 4; with -n 1 all four strands are searched from one read
    "c2": dict(kw=dict(s=16, v=4, I=4, S=1, r=1), pe=False, L=100, kind=0, n=131072),
    "c2_n1": dict(kw=dict(s=16, v=4, I=4, S=1, r=1, n=1), pe=False, L=100, kind=0, n=65536),
    # C5: 2x144 with 3' adapters and low-quality tails, -A <adapter> -q 20 (variable read lengths after trimming)
    "c5": dict(kw=dict(s=16, v=6, I=4, m=28, x=500, S=1, r=1, pairend=1, q=20, A=[ADAPTER]), pe=True, L=144, kind=1, n=65536),
    # C4: RRBS -D C-CGG (seed 12, interval 1 forced), 1x75 reads at digestion sites; site tables + {tag, loc} index of the whole genome
    "c4": dict(kw=dict(D="C-CGG", S=1, r=1), pe=False, L=75, kind=2, n=65536),
}


@pytest.fixture(scope="module", params=sorted(OTHER))
def other(request, oracle, oracle_wgbs):
    name = request.param
    cfg = OTHER[name]
    ref = B.RefSeq(B.make_params(**cfg["kw"])).synthetic(HG38, seed=38).CreateIndex()
    al = (B.PairAlign if cfg["pe"] else B.SingleAlign)(ref, cfg["n"])
    al.synth_reads(cfg["n"], cfg["L"], seed=17, kind=cfg["kind"])
    al.Do_Batch()
    res = tuple(x.copy() for x in al.results())
    cnt = al.counters().copy()
    HEAVY[name] = (int(al.heavy_units()), int(al.redo_units()))   # of THIS run
    oref = _oracle_ref(name, cfg, ref, oracle, oracle_wgbs)   # (built once for the tests of this config: C4's from the genome text is the costly one)
    yield name, cfg, ref, al, res, cnt, oref
    oref.free()
    al.close()
    ref.close()


def test_other_configs_closure_idempotence_partition(other):
    name, cfg, ref, al, res, cnt, _ = other
    n = cfg["n"]
    assert int(cnt[4]) == n
    assert ref.n_words > 190_000_000 and ref.n_entries > (1_000_000 if name == "c4" else 1_400_000_000)
    al.reset_counters()
    al.Do_Batch()
    res2 = al.results()
    for a, b in zip(res, res2):
        assert a.tobytes() == b.tobytes()
    assert np.array_equal(al.counters()[:7], cnt[:7])
    al.run_range(n // 2, n // 2, sync=True)
    al.run_range(0, n // 2, sync=True)
    for a, b in zip(res, al.results()):
        assert a.tobytes() == b.tobytes()
    al.set_work_counters(False)   # (what the command line runs: records must not depend on the counters)
    try:
        al.reset_counters()
        al.Do_Batch()
        for a, b in zip(res, al.results()):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(al.counters()[4:7], cnt[4:7])
    finally:
        al.set_work_counters(True)
    if cfg["pe"]:
        out = res[0]
        placed = (out["unpaired_out"] == 0).mean()
        assert placed > 0.9, placed            # trimmed pairs still pair up
        assert len(np.unique(out["a"]["len"])) > 20   # trimming really produced a spread of read lengths
    else:
        hits = res[0]
        assert (hits["n_best"] > 0).mean() > (0.85 if name != "c4" else 0.8)


def _oracle_ref(name, cfg, ref, oracle, oracle_wgbs):
    kw = cfg["kw"]
    if name == "c4":   # RRBS: the oracle's OWN packing, site tables and index of the genome text
        text = _genome_text(ref)
        oref = oracle.OracleRef(oracle.make_params(**kw), fasta_text=text)
        del text
        assert sum(len(oref.sites(c)) for c in range(ref.n_chr)) == sum(len(ref.sites(c)) for c in range(ref.n_chr))
        assert np.array_equal(oref.sites(3), ref.sites(3))
        assert np.array_equal(oref.rrbs_entries(), ref.index()[2])
        return oref
    oracle_wgbs.check(ref, name)   # this config's own GPU-built reference + index against the oracle's build
    return oracle_wgbs.ref_for(kw)


def test_other_configs_whole_batch_equals_oracle(other, oracle):
    """every unit of the batch re-aligned by the oracle's batch driver against the oracle's OWN build of reference + index from
    the 3.1 GB genome text (WGBS and RRBS alike; the device's copy is compared with it first) — every record field and the four
    work counters; C5 also in exact mode (bsx_batch_set_leak_exact) against the oracle's `-p 1` state (leak_mode 1)"""
    import wholebatch as W
    name, cfg, ref, al, res, cnt, oref = other
    kw, n = cfg["kw"], cfg["n"]
    nclass = kw.get("v", 2) + 1
    quals = cfg["kind"] == 1
    ores, ocnt, t_cpu = W.run_oracle(oracle, oref, al, cfg["pe"], quals, n)
    if cfg["pe"]:
        bad, info = W.compare_pe(ores, res[0], res[1], res[2], res[3], nclass)
    else:
        bad, info = W.compare_se(ores, res[0], res[1], nclass)
    rec = dict(info, units=n, oracle_s=round(t_cpu, 1), counters_gpu=[int(x) for x in cnt[:4]], counters_oracle=ocnt, mismatching_fields=bad,
               options={k: v for k, v in kw.items()}, heavy_units=HEAVY[name][0], redo_units=HEAVY[name][1],
               reference="oracle-built from the genome text")
    if name == "c5":   # the only BASELINE config whose reads leak planner state ((len - I + 1) % S == 0 after trimming)
        ex = B.PairAlign(ref, n).set_leak_exact()
        try:
            ex.synth_reads(n, cfg["L"], seed=17, kind=cfg["kind"])
            ex.Do_Batch()
            eres = ex.results()
            ecnt = [int(x) for x in ex.counters()[:4]]
        finally:
            ex.close()
        lres, lcnt, t_leak = W.run_oracle(oracle, oref, al, True, True, n, leak_mode=1)
        ebad, _ = W.compare_pe(lres, eres[0], eres[1], eres[2], eres[3], nclass)
        S, I = kw["s"], kw["I"]
        leaky = sum(int((((lres[m]["len"] - I + 1) % S == 0) & (lres[m]["filtered"] == 0)).sum()) for m in ("a", "b"))
        differ = int((eres[0].tobytes() != res[0].tobytes()))
        rec["exact_mode"] = dict(oracle_s=round(t_leak, 1), counters_gpu=ecnt, counters_oracle=lcnt, mismatching_fields=ebad, leaky_reads=leaky,
                                 records_differ_from_default_mode=bool(differ))
        W.record(name, rec)
        assert leaky > n // 50
        assert not ebad, ebad
        assert ecnt == lcnt
    else:
        W.record(name, rec)
    assert not bad, bad
    assert [int(x) for x in cnt[:4]] == ocnt


BENCH_STEP = {"c2": "se", "c4": "rrbs", "c5": "trim"}   # this module's config -> bench.py's mode


@pytest.mark.parametrize("other", sorted(BENCH_STEP), indirect=True)
def test_bench_step_equals_the_oracle(other, oracle):
    """bench.py's own regime for C2 / C4 / C5: a batch that holds two of the mode's steps (reads as the bench's ring makes them: seed 3, unit ids
    from 0), created under the mode's starting pools with the work counters off, runs its SECOND step (unit ids at and above the step size reach
    the pick RNG and the mate indexing).  32 blocks of 4 096 units and ~256 deferred units taken evenly over the deferred list are re-aligned by
    the oracle against its own reference + index: every record field.  The test also shows that it ran the bench's regime: the pools as
    started, several rounds of deferred units (C4: at least 10; C5: at least 2) with compared units in every round.  C2 and C5 then run the same
    step on as many batches at once as the bench keeps in flight: byte-identical records.  (C4 is left out there: three RRBS batches plan 0.88
    of the device.)"""
    import threading
    import wholebatch as W
    name, cfg, ref, _, _, _, oref = other
    mode = BENCH_STEP[name]
    M, units, nfl, limits = W.bench_mode(mode)
    assert M["kw"] == cfg["kw"] and M["pe"] == cfg["pe"] and M["L"] == cfg["L"] and M["kind"] == cfg["kind"]
    batches = [W.bench_batch(ref, mode, 2 * units)]
    try:
        batches[0].synth_reads(2 * units, M["L"], seed=3, kind=M["kind"])
        bad, info = W.bench_step_blocks(oracle, oref, batches[0], mode, units)
        if mode != "rrbs":
            lone = [x[units:2 * units].tobytes() for x in batches[0].results()]
            for _ in range(nfl - 1):
                batches.append(W.bench_batch(ref, mode, 2 * units))
                batches[-1].synth_reads(2 * units, M["L"], seed=3, kind=M["kind"])

            def work(j):
                batches[j].run_range(units, units, sync=True)

            th = [threading.Thread(target=work, args=(j,)) for j in range(1, nfl)]
            for t in th:
                t.start()
            work(0)
            for t in th:
                t.join()
            info["in_flight"] = dict(batches=nfl, pool_sizes=[list(b.pool_sizes()) for b in batches], heavy_units=[int(b.heavy_units()) for b in batches],
                                     identical=[[x[units:2 * units].tobytes() for x in b.results()] == lone for b in batches])
    finally:
        for b in batches:
            b.close()
    W.record(f"bench_step_{name}", info)
    assert info["pool_sizes"] == list(limits), (info["pool_sizes"], limits)   # halved pools: not the bench's regime
    heavy, rounds = info["heavy_units"], info["rounds"]
    assert info["rounds_covered"] == rounds, info["deferred_compared_per_round"]
    if mode == "rrbs":
        assert heavy > units // 2 and rounds >= 10, (heavy, rounds)
    if mode == "trim":
        assert rounds >= 2, (heavy, rounds)
    assert info["deferred_units_compared"] >= 1000, info["deferred_units_compared"]
    placed = info["paired_out" if M["pe"] else "placed"] / info["units_compared"]
    assert placed > {"se": 0.85, "rrbs": 0.8, "trim": 0.9}[mode], placed   # (the levels of test_other_configs_closure_idempotence_partition)
    assert not bad, bad
    if mode != "rrbs":
        assert all(info["in_flight"]["identical"]), info["in_flight"]
