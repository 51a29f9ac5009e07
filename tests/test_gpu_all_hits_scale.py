"""All hits at a size where slabs are reused and the heavy pipeline runs: 2^19 units on the hg38-sized synthetic genome (the whole-batch tests'), pools of
the heavy pipeline small enough for several rounds, the spans of EVERY emitting unit (more than a thousand, hundreds of them deferred units from every round) compared with the oracle's best-class lists.  Needs an MI355X.

The oracle aligns against the device's own packed reference and index, pulled back and wrapped (tests/test_gpu_fullsize.py holds every word, offset and entry
of them to the oracle's own build from the genome text; building that a second time costs a minute of GPU-box time and proves nothing new here).

Single-end: C2's options and reads (1x100).  Paired: C3's options with 2x64 reads.  C3's own 2x144 pairs almost never emit on this genome (3 units of
4 194 304 in a bench step, tools/all_hits_cost.py; with the mates crossed 43 of 524 288): long mates pin each other down.  At 64 nt, 1.4 % of the pairs
emit — most of them the lists of the mates of an unreported pair, some dozens a pair list — and nearly all of those go through the heavy pipeline.
More than 2 048 emitting units: every unit with a pair list and 2 048 of the others, taken evenly."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bsmap_amd as B
import wholebatch as W
from test_gpu_all_hits import check_picks, check_spans, oracle_pe_lists, oracle_se_lists
from test_gpu_fullsize import HG38

pytestmark = pytest.mark.gpu

N = 1 << 19
CFG = {
    "se": dict(kw=dict(s=16, v=4, I=4, S=1, r=1), pe=False, L=100, limits=(512, 65536)),
    "pe": dict(kw=dict(s=16, v=6, I=4, m=28, x=500, S=1, r=1, pairend=1), pe=True, L=64, limits=(512, 65536)),
}
MIN_COMPARED, MIN_HEAVY, MIN_ROUNDS = 1000, 256, 3


@pytest.fixture(scope="module")
def genome_arrays():
    """the device-built reference + index (-s 16 -I 4: shared by both configs) as host arrays for OracleRef.wrap"""
    ref = B.RefSeq(B.make_params(**CFG["se"]["kw"])).synthetic(HG38, seed=38).CreateIndex(context=0)
    f, c = ref.words()
    a, s, r = ref.info()
    off, nf, ent = ref.index()
    ref.close()
    return f, c, a, s, r, off, nf, ent


def _batch(ref, cfg, n=N):
    assert B.lib().bsx_set_heavy_limits(*cfg["limits"]) == 0
    try:
        al = (B.PairAlign if cfg["pe"] else B.SingleAlign)(ref, n)
    finally:
        B.lib().bsx_set_heavy_limits(0, 0)
    return al


def _load(al, cfg, reads=None):
    """synthetic reads (seed 11), or the host copies of an earlier call.  Returns the host copies (uint8 [N, L] per mate)"""
    if reads is None:
        al.synth_reads(N, cfg["L"], seed=11)
        reads = []
        for m in range(2 if cfg["pe"] else 1):
            b, o = al.download_reads(m)
            assert np.array_equal(np.diff(o.astype(np.int64)), np.full(N, cfg["L"]))
            reads.append(b[:N * cfg["L"]].reshape(N, cfg["L"]))
    off = (np.arange(N + 1, dtype=np.uint64) * cfg["L"])
    bufs = [np.ascontiguousarray(r).reshape(-1) for r in reads]
    if cfg["pe"]:
        al.ImportBatchReads((bufs[0], off), (bufs[1], off))
    else:
        al.ImportBatchReads((bufs[0], off))
    return reads


@pytest.fixture(scope="module", params=["se", "pe"])
def scale(request, oracle, genome_arrays):
    cfg = CFG[request.param]
    ref = B.RefSeq(B.make_params(**cfg["kw"])).synthetic(HG38, seed=38).CreateIndex()
    oref = oracle.OracleRef.wrap(oracle.make_params(**cfg["kw"]), *genome_arrays)
    al = _batch(ref, cfg)
    reads = _load(al, cfg)
    al.Do_Batch()
    plain = tuple(None if x is None else x.copy() for x in al.results())
    al.set_all_hits(1 << 20)   # a first run only to learn the need
    al.Do_Batch()
    need, _ = al.all_hits_need()
    al.set_all_hits(need)
    al.Do_Batch()
    spans, pool = al.all_hits()
    yield request.param, cfg, ref, oref, al, reads, plain, spans, pool, oracle
    al.close()
    oref.free()
    ref.close()


def test_spans_of_a_large_batch_equal_the_oracle(scale):
    name, cfg, ref, oref, al, reads, plain, spans, pool, O = scale
    for a, b in zip(plain, al.results()):
        assert (a is None and b is None) or a.tobytes() == b.tobytes(), "a pool changed the records"
    need, _ = check_spans(al, spans, pool)
    heavy = al.heavy_list().astype(np.int64)
    pools = al.pool_sizes()
    rounds = -(-len(heavy) // pools[0])
    emitting = (spans["n"] > 0).any(axis=1)
    hv = heavy[emitting[heavy]]                                  # emitting deferred units, in the order they were deferred (= by round)
    is_heavy = np.zeros(N, bool)
    is_heavy[heavy] = True
    rest = np.nonzero(emitting & ~is_heavy)[0]
    pick_h, pick_r = hv, rest                                    # every emitting unit (the oracle takes seconds for them on 16 CPUs) ...
    if len(hv) + len(rest) > 2048:                               # ... or every unit with a pair list and 2 048 of the others, taken evenly
        both = np.sort(np.concatenate([hv, rest]))
        some = set(both[np.unique(np.linspace(0, len(both) - 1, 2048).round().astype(np.int64))].tolist()) | set(np.nonzero(spans["n"][:, 2] > 0)[0].tolist())
        pick_h, pick_r = np.array([u for u in hv if u in some], np.int64), np.array([u for u in rest if u in some], np.int64)
    units = [int(u) for u in np.concatenate([pick_h, pick_r])]
    quiet = [int(u) for u in np.nonzero(~emitting)[0][::max(1, N // 256)]]   # and some that must stay silent
    tl = threading.local()
    made = []

    def one(u):
        if not hasattr(tl, "al"):
            tl.al = O.OracleAligner(oref, leak_mode=0)
            made.append(tl.al)
        if cfg["pe"]:
            want = oracle_pe_lists(tl.al, tl.al.pe(u, reads[0][u].tobytes().decode(), reads[1][u].tobytes().decode()))
        else:
            want = oracle_se_lists(tl.al, tl.al.se(u, reads[0][u].tobytes().decode()))
        return B.all_hits_lists(spans[u], pool) == tuple(want)

    with ThreadPoolExecutor(W.usable_cpus()) as ex:
        ok = list(ex.map(one, units + quiet))
    for a in made:
        a.free()
    bad = [u for u, k in zip(units + quiet, ok) if not k]
    print(f"{name}: {int(emitting.sum())} emitting units of {N}, {need} words; compared {len(units)} emitting ({len(pick_h)} deferred of {len(hv)} emitting deferred, "
          f"{len(heavy)} deferred in all, {rounds} rounds of {pools[0]}) and {len(quiet)} silent units with the oracle; mismatches {len(bad)}")
    assert not bad, bad[:10]
    assert len(units) >= MIN_COMPARED and len(pick_h) >= MIN_HEAVY and rounds >= MIN_ROUNDS, (len(units), len(pick_h), rounds)
    n_pair_lists = int((spans["n"][:, 2] > 0).sum())
    assert not cfg["pe"] or n_pair_lists >= 8, n_pair_lists
    assert check_picks("pe" if cfg["pe"] else "se", plain, spans, pool, cfg["kw"]["S"]) >= int(emitting.sum())


def _lists_digest(spans, pool):
    """per-unit content of the spans, independent of where the units landed in the pool"""
    out = []
    for u in np.nonzero((spans["n"] > 0).any(axis=1))[0]:
        out.append((int(u), B.all_hits_lists(spans[u], pool)))
    return out


def test_three_batches_at_once_give_the_same_lists(scale):
    name, cfg, ref, oref, al, reads, plain, spans, pool, O = scale
    want = _lists_digest(spans, pool)
    need, _ = al.all_hits_need()
    others = [_batch(ref, cfg) for _ in range(3)]
    got = [None] * 3
    try:
        for o in others:
            _load(o, cfg, reads)
            o.set_all_hits(need)

        def work(j):
            others[j].Do_Batch()
            s, p = others[j].all_hits()
            assert others[j].all_hits_need() == (need, 0)
            got[j] = (_lists_digest(s, p), others[j].results()[0].tobytes())

        th = [threading.Thread(target=work, args=(j,)) for j in range(3)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for j in range(3):
            assert got[j] is not None and got[j][1] == plain[0].tobytes() and got[j][0] == want, j
    finally:
        for o in others:
            o.close()


def test_overflow_at_scale(scale):
    name, cfg, ref, oref, al, reads, plain, spans, pool, O = scale
    want = dict(_lists_digest(spans, pool))
    need, _ = al.all_hits_need()
    al.set_all_hits(need // 4)
    al.Do_Batch()
    assert al.results()[0].tobytes() == plain[0].tobytes(), "a full pool changed the records"
    s2, p2 = al.all_hits()
    need2, dropped = check_spans(al, s2, p2, expect_dropped=1)
    assert need2 == need and dropped > 0
    assert np.array_equal(s2["n"], spans["n"]) and np.array_equal(s2["n_fwd"], spans["n_fwd"]), "a dropped span lost its counts"
    kept = 0
    for u, lists in _lists_digest(s2, p2):
        if any(x is None for x in lists):
            assert all(x is None or x == [] for x in lists), u      # a unit is in the pool whole or not at all
            continue
        assert lists == want[u], u
        kept += 1
    assert kept == len(want) - dropped and kept > 0
    al.set_all_hits(need2)
    al.Do_Batch()
    s3, p3 = al.all_hits()
    assert check_spans(al, s3, p3) == (need, 0)
    assert dict(_lists_digest(s3, p3)) == want
