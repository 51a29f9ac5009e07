"""Whole-batch comparison of the records the C ABI returns with the oracle's batch driver (tests only): every field of every
unit plus the four work counters that the roofline numerator is made of.  Returns {field: number of mismatching units}."""
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def usable_cpus():
    import bench
    return bench.usable_cpus()


def _chk(bad, name, x, y):
    x, y = np.asarray(x), np.asarray(y)
    n = int((x != y).sum()) if x.shape == y.shape else -1
    if n:
        bad[name] = n


def compare_se(ores, hits, cc, nclass):
    bad = {}
    _chk(bad, "filtered", ores["filtered"] != 0, (hits["flags"] & 1) != 0)
    _chk(bad, "len", ores["len"], hits["len"])
    _chk(bad, "raw_len", ores["raw_len"], hits["raw_len"])
    ok = ores["filtered"] == 0
    _chk(bad, "max_snp", ores["read_max_snp_num"][ok], hits["max_snp"][ok])
    _chk(bad, "seedseg", ores["seedseg_num"][ok], hits["seedseg"][ok])
    _chk(bad, "n_hit", ores["n_hit"][ok][:, :nclass], cc["n_hit"][ok][:, :nclass])
    _chk(bad, "n_chit", ores["n_chit"][ok][:, :nclass], cc["n_chit"][ok][:, :nclass])
    _chk(bad, "n_best", np.maximum(ores["n_best"], 0)[ok], hits["n_best"][ok])
    has = ok & (ores["n_best"] > 0)
    for f in ("chr", "loc", "best_class"):
        _chk(bad, f, ores[f][has], hits[f][has])
    _chk(bad, "chain", ores["chain"][has] != 0, (hits["flags"][has] & 2) != 0)
    n_limit = int(((hits["flags"] & 4) != 0).sum())   # BSX_F_LIMIT: the one capacity the reference does not have (include/bsx.h) — never reached
    if n_limit:
        bad["BSX_F_LIMIT"] = n_limit
    return bad, {"placed": int(has.sum()), "filtered": int((~ok).sum()), "flagged_BSX_F_LIMIT": n_limit}


def compare_pe(ores, out, ca, cb, npairs, nclass):
    bad = {}
    _chk(bad, "paired", ores["paired"], out["paired"])
    both = (ores["a"]["filtered"] == 0) & (ores["b"]["filtered"] == 0)
    _chk(bad, "n_pairs", ores["n_pairs"][both][:, :2 * nclass - 1], npairs[both][:, :2 * nclass - 1])
    up = (ores["tmp"] == 1) | (ores["paired"] == 0)
    _chk(bad, "unpaired_out", up, out["unpaired_out"] != 0)
    pr = ~up
    for f in ("chain", "na", "nb", "insert", "a_chr", "a_loc", "b_chr", "b_loc"):
        _chk(bad, "pick." + f, ores["pick"][f][pr], out[f][pr])
    pd = ores["paired"] > 0
    _chk(bad, "pair_class", ores["pair_class"][pd], out["pair_class"][pd])
    _chk(bad, "pair_n", ores["pair_n"][pd], out["n_pairs"][pd])
    for m, cnts in (("a", ca), ("b", cb)):
        o, g = ores[m], out[m]
        _chk(bad, m + ".filtered", o["filtered"] != 0, (g["flags"] & 1) != 0)
        _chk(bad, m + ".len", o["len"], g["len"])
        _chk(bad, m + ".raw_len", o["raw_len"], g["raw_len"])
        ok = o["filtered"] == 0
        _chk(bad, m + ".max_snp", o["read_max_snp_num"][ok], g["max_snp"][ok])
        _chk(bad, m + ".seedseg", o["seedseg_num"][ok], g["seedseg"][ok])
        _chk(bad, m + ".n_hit", o["n_hit"][ok][:, :nclass], cnts["n_hit"][ok][:, :nclass])
        _chk(bad, m + ".n_chit", o["n_chit"][ok][:, :nclass], cnts["n_chit"][ok][:, :nclass])
        sel = up & ok & (o["n_best"] > 0)
        _chk(bad, m + ".n_best", o["n_best"][sel], g["n_best"][sel])
        for f in ("chr", "loc", "best_class"):
            _chk(bad, f"{m}.{f}", o[f][sel], g[f][sel])
        _chk(bad, m + ".chain", o["chain"][sel] != 0, (g["flags"][sel] & 2) != 0)
    return bad, {"paired_out": int(pr.sum()), "filtered_mates": int((ores["a"]["filtered"] != 0).sum() + (ores["b"]["filtered"] != 0).sum())}


def run_oracle(O, oref, al, pe, quals, K, leak_mode=0):
    """the oracle's batch driver over units [0, K) of device batch `al` on every CPU this process may use"""
    b1, o1 = al.download_reads(0)
    q1 = al.download_quals(0) if quals else None
    e1 = int(o1[K])
    t0 = time.time()
    if pe:
        b2, o2 = al.download_reads(1)
        q2 = al.download_quals(1) if quals else None
        e2 = int(o2[K])
        res, cnt = O.pe_batch(oref, b1[:e1], o1[:K + 1].copy(), b2[:e2], o2[:K + 1].copy(), q1[:e1] if quals else None, q2[:e2] if quals else None,
                              threads=usable_cpus(), leak_mode=leak_mode)
    else:
        res, cnt = O.se_batch(oref, b1[:e1], o1[:K + 1].copy(), q1[:e1] if quals else None, threads=usable_cpus(), leak_mode=leak_mode)
    return res, [int(x) for x in cnt], time.time() - t0


def bench_mode(mode):
    """bench.py's own settings for `mode`: (MODES entry, units per step, batches in flight, starting pools).  Where MODE_DEFAULTS names no pools,
    the library's starting sizes for one step, as bench.memory_plan and the timed region set them."""
    import bench
    import bsmap_amd as B
    M = bench.MODES[mode]
    units, nfl, limits = bench.mode_defaults(mode)
    if limits is None:
        limits = B.default_heavy_limits(B.make_params(**M["kw"]), units, M["pe"])
    return M, units, nfl, tuple(limits)


def bench_batch(ref, mode, max_units):
    """a device batch as bench.py's timed region has it: created under the mode's starting pools (which bsx_batch_create reads; the library's
    defaults are restored afterwards) and with the work counters off"""
    import bsmap_amd as B
    M, _, _, limits = bench_mode(mode)
    L = B.lib()
    assert L.bsx_set_heavy_limits(*limits) == 0
    try:
        al = (B.PairAlign if M["pe"] else B.SingleAlign)(ref, max_units)
    finally:
        L.bsx_set_heavy_limits(0, 0)
    return al.set_work_counters(False)


def bench_step_blocks(oracle, oref, al, mode, first, n_blocks=32, blk=4096, n_extra=256):
    """Run one bench step, units [first, first + units per step) of `al` (a bench_batch whose reads carry unit ids from 0), and re-align with the
    oracle against `oref`: n_blocks blocks of blk consecutive units spread over the step, off the power-of-two grid, and about n_extra deferred
    units taken evenly by POSITION in the deferred list, each alone (the pick RNG is a function of the unit's own index).  The deferred list is in
    k_align's atomicAdd order and the heavy pipeline takes it in that order, per_round = ceil(n_heavy / n_rounds) units a round: a unit's round
    is its position // per_round.  Returns ({field: mismatching units}, info)."""
    M, n, _, limits = bench_mode(mode)
    pe, kw, quals = M["pe"], M["kw"], M["kind"] == 1
    nclass = kw.get("v", 2) + 1
    assert first + n <= al.n
    t0 = time.time()
    al.run_range(first, n, sync=True)
    t_gpu = time.time() - t0
    res = al.results()
    heavy, redo, pools = int(al.heavy_units()), int(al.redo_units()), tuple(al.pool_sizes())
    hlist = al.heavy_list().astype(np.int64)
    assert len(hlist) == heavy, (len(hlist), heavy)
    assert heavy == 0 or (hlist.min() >= first and hlist.max() < first + n), (first, n, int(hlist.min()), int(hlist.max()))
    n_rounds = -(-heavy // pools[0])
    per_round = -(-heavy // n_rounds) if n_rounds else 1
    round_of = np.full(n, -1, np.int64)   # by unit of the step: the round that took it, -1 = not deferred
    round_of[hlist - first] = np.arange(heavy) // per_round
    spans = [(first + k * (n // n_blocks) + 17 * k, first + k * (n // n_blocks) + 17 * k + blk) for k in range(n_blocks)]
    assert spans[-1][1] <= first + n
    pos = np.unique(np.linspace(0, heavy - 1, min(n_extra, heavy)).round().astype(np.int64))
    extra = [int(u) for u in hlist[pos] if not any(lo <= u < hi for lo, hi in spans)]
    in_blocks = np.concatenate([round_of[lo - first:hi - first] for lo, hi in spans])
    in_blocks = in_blocks[in_blocks >= 0]
    per_round_compared = np.bincount(np.concatenate([in_blocks, round_of[np.array(extra, np.int64) - first]]), minlength=n_rounds)
    reads = [al.download_reads(m) for m in range(2 if pe else 1)]
    qual = [al.download_quals(m) if quals else None for m in range(2 if pe else 1)]

    def check(span):
        lo, hi = span
        mates = []
        for (b, o), q in zip(reads, qual):
            e0, e1 = int(o[lo]), int(o[hi])
            mates += [b[e0:e1], (o[lo:hi + 1] - o[lo]).copy(), q[e0:e1] if quals else None]
        if pe:
            ores, _ = oracle.pe_batch(oref, mates[0], mates[1], mates[3], mates[4], mates[2], mates[5], first_index=lo, threads=1)
            bad, info = compare_pe(ores, *(x[lo:hi] for x in res), nclass)
            return bad, info["paired_out"]
        ores, _ = oracle.se_batch(oref, mates[0], mates[1], mates[2], first_index=lo, threads=1)
        bad, info = compare_se(ores, res[0][lo:hi], res[1][lo:hi], nclass)
        return bad, info["placed"]

    # one-thread oracle calls over 512 units of a block or one deferred unit, as many at a time as there are CPUs (the calls release the GIL; a
    # unit's records do not depend on the units aligned before it): one after the other, the deferred units alone left all CPUs but one idle
    calls = [(a, min(a + 512, hi)) for lo, hi in spans for a in range(lo, hi, 512)] + [(u, u + 1) for u in extra]
    bad_all, placed = {}, 0
    t0 = time.time()
    with ThreadPoolExecutor(usable_cpus()) as ex:
        for bad, k in ex.map(check, calls):
            placed += k
            for f, c in bad.items():
                bad_all[f] = bad_all.get(f, 0) + c
    t_cpu = time.time() - t0
    info = dict(units_in_batch=int(al.n), units_in_step=n, first_unit=first, units_compared=blk * n_blocks + len(extra), blocks=n_blocks, block_units=blk,
                heavy_units=heavy, redo_units=redo, deferred_units_compared=len(in_blocks) + len(extra), deferred_in_blocks=len(in_blocks), deferred_alone=len(extra),
                rounds=n_rounds, units_per_round=per_round, rounds_covered=int((per_round_compared > 0).sum()),
                deferred_compared_per_round=[int(x) for x in per_round_compared], pool_sizes=list(pools), starting_pools=list(limits),
                oracle_s=round(t_cpu, 1), do_batch_s=round(t_gpu, 3), mismatching_fields=bad_all, options=kw, work_counters=False,
                reference="oracle-built from the genome text")
    info["paired_out" if pe else "placed"] = placed
    return bad_all, info


ROUND = "r07"


def record(name, info):
    """profiles/<round>_validate_<cfg>.json is a copy of what this writes on the GPU box (gpurun_out/ travels back)"""
    import bench
    d = os.environ.get("BSX_VALIDATE_DIR") or os.path.join(ROOT, "gpurun_out", "validate")
    os.makedirs(d, exist_ok=True)
    info = dict(info, config=name, lib_sha16=bench.lib_sha16(), oracle_threads=usable_cpus())
    with open(os.path.join(d, f"{ROUND}_validate_{name}.json"), "w") as f:
        json.dump(info, f, indent=1, sort_keys=True)
