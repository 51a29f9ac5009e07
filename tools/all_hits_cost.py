#!/usr/bin/env python3
"""What the all-hits pool (include/bsx.h: bsx_batch_set_all_hits) costs and wants on the bench workloads: for C2 (--mode se) and C3 (--mode pe), one
bench-sized step on the hg38-sized synthetic genome, ONE batch in flight (bench.py's headline runs two or three: these are serial step times, to be
compared with each other only), work counters off as in the bench's timed region.

Prints one JSON line per mode: ms per step without and with a pool (median of --reps runs of the same step), the words the step wants, units that
emit, words per unit of the step, units dropped at --pool-words (0 = twice the need: nothing dropped), and how many of the emitting units went
through the heavy pipeline.  DESIGN.md "All hits" quotes its output.

    python tools/all_hits_cost.py --mode se --mode pe [--units N] [--pool-words W]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import bsmap_amd as B  # noqa: E402


def step_ms(al, n, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        al.run_range(0, n, sync=True)
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def measure(mode, units, pool_words, reps):
    M = bench.MODES[mode]
    n = units or bench.mode_defaults(mode)[0]
    limits = bench.mode_defaults(mode)[2] or B.default_heavy_limits(B.make_params(**M["kw"]), n, M["pe"])
    ref = B.RefSeq(B.make_params(**M["kw"])).synthetic(bench.HG38, seed=38).CreateIndex()
    assert B.lib().bsx_set_heavy_limits(*limits) == 0
    try:
        al = (B.PairAlign if M["pe"] else B.SingleAlign)(ref, n)
    finally:
        B.lib().bsx_set_heavy_limits(0, 0)
    al.set_work_counters(False)
    al.synth_reads(n, M["L"], seed=11, kind=M["kind"])
    al.run_range(0, n, sync=True)   # warm-up
    off = step_ms(al, n, reps)
    al.set_all_hits(1 << 20)        # a first run only to learn the need
    al.run_range(0, n, sync=True)
    need, _ = al.all_hits_need()
    al.set_all_hits(max(2 * need, 1024))
    al.run_range(0, n, sync=True)
    on = step_ms(al, n, reps)
    need2, dropped = al.all_hits_need()
    assert need2 == need and dropped == 0, (need, need2, dropped)
    spans, pool = al.all_hits()
    emitting = (spans["n"] > 0).any(axis=1)
    heavy = al.heavy_list().astype(np.int64)
    words = (spans["n"][:, :2].astype(np.int64) * 2).sum(axis=1) + spans["n"][:, 2].astype(np.int64) * 6
    assert int(words.sum()) == need == len(pool)
    dropped_at = None
    if pool_words:
        al.set_all_hits(pool_words)
        al.run_range(0, n, sync=True)
        dropped_at = al.all_hits_need()[1]
    out = dict(mode=mode, config=M["tag"], units=n, batches_in_flight=1, reps=reps, ms_per_step_off=[round(x, 2) for x in off], ms_per_step_on=[round(x, 2) for x in on],
               median_off=round(statistics.median(off), 2), median_on=round(statistics.median(on), 2), need_words=int(need), words_per_unit=need / n,
               units_emitting=int(emitting.sum()), largest_unit_words=int(words.max()), heavy_units=int(len(heavy)), heavy_units_emitting=int(emitting[heavy].sum()),
               pool_words_tried=pool_words or None, units_dropped_at_that_pool=dropped_at, lib_sha16=bench.lib_sha16())
    print(json.dumps(out), flush=True)
    al.close()
    ref.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", action="append", choices=sorted(bench.MODES))
    ap.add_argument("--units", type=int, default=0, help="units of the step (0: the bench's step for the mode)")
    ap.add_argument("--pool-words", type=int, default=0, help="also count the units a pool of this size drops")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    for mode in a.mode or ["se", "pe"]:
        measure(mode, a.units, a.pool_words, a.reps)


if __name__ == "__main__":
    main()
