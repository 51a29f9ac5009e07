#!/usr/bin/env python3
"""Throughput of the methylation pile-up kernels (bsx_meth_add) on an hg38-sized random reference: N alignments of L nt
at uniform positions, all four strands, reads = reference letters with bisulfite-like conversion.  Prints one JSON line;
run under `rocprofv3 --kernel-trace --stats` for the kernel-only times.  `--ct-snp correct|skip` turns the C/T-SNP mode on (one more 64-bit cell per
reference letter, reverse calls in the pile-up, the SNP tests in the report).  `--wig-bin B[,B...]` times bsx_meth_bins over all chromosomes and
`--regions N,LEN[;N,LEN...]` bsx_meth_regions over N intervals of LEN nt at uniform positions (made here, no file), both with their copies to the host and
`--repeat` times each, in the order given (the order of their launches in a kernel trace).  `--nonconv-filter N`, `--read-stats` and `--pdr` (with
`--pdr-min-cpg K`) turn the per-read pass on (k_meth_reads ahead of the pile-up: DESIGN §3.10); the JSON line then carries the dropped reads, the histogram's
totals and the PDR rows.  (The reads here keep 30 % of ALL their cytosines, whatever the context: nearly every read has three methylated non-CpG calls, so
`--nonconv-filter 3` drops nearly all of them and the pile-up behind it has little left to do; a threshold such as 40 drops nearly none.)  `--epi` turns the
epiallele tally on (k_meth_epi behind the per-read pass: DESIGN §3.11) and times the build of the CpG index (bsx_meth_n_cpg on the whole reference, ahead of
the first add) and bsx_meth_epi_report_chr over all chromosomes; the JSON line then carries the CpGs and the epiallele rows.  `--diff` makes a second handle
over the same reference, fed the same alignments converted under another seed (sample B), and times bsx_meth_diff_report_chr over all chromosomes (with
`--diff-delta PERMILLE` as its filter) and, for every `--regions` entry, bsx_meth_diff_regions on the same intervals right behind bsx_meth_regions (DESIGN
§3.12): in a kernel trace of the run k_diff_count / k_diff_emit / k_meth_fisher stand beside k_meth_count / k_meth_emit, and k_meth_diff_regions beside
k_meth_regions; the JSON line carries the rows and the host-side times.  (Not with --ct-snp: a diff call needs the mode off.)  With `--fdr` (needs --diff) it also
times bsx_meth_diff_report_all (the genome-wide store with its q-values: the radix sort, k_bh_keys / k_bh_ratio / k_bh_scatter and the running minimum stand in
the trace behind one k_diff_count / k_diff_emit per chromosome) and bsx_meth_diff_dmrs over it (k_cand_* / k_head_* / k_dmr_runs; `--dmr-max-q Q`, default 0.05,
with the defaults of methdiff for the rest).
usage: meth_bench.py [--aln 16777216] [--len 100] [--ct-snp MODE] [--nonconv-filter N] [--read-stats] [--pdr] [--epi] [--diff [--fdr]] [--wig-bin B,...] [--regions N,LEN;...] [--repeat R]"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bsmap_amd as B
from bsmap_amd import methratio as MR


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aln", type=int, default=16 << 20)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--genome", type=float, default=1.0)
    ap.add_argument("--ct-snp", dest="ct_snp", choices=MR.CT_SNP_MODES, default="no-action")
    ap.add_argument("--wig-bin", dest="wig_bin", default="")
    ap.add_argument("--regions", dest="regions", default="")
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--nonconv-filter", dest="nonconv_filter", type=int, default=0)
    ap.add_argument("--read-stats", dest="read_stats", action="store_true")
    ap.add_argument("--pdr", dest="pdr", action="store_true")
    ap.add_argument("--pdr-min-cpg", dest="pdr_min_cpg", type=int, default=4)
    ap.add_argument("--epi", dest="epi", action="store_true")
    ap.add_argument("--diff", dest="diff", action="store_true")
    ap.add_argument("--diff-delta", dest="diff_delta", type=int, default=0)
    ap.add_argument("--fdr", dest="fdr", action="store_true")
    ap.add_argument("--dmr-max-q", dest="dmr_max_q", type=float, default=0.05)
    a = ap.parse_args()
    if a.fdr and not a.diff:
        ap.error("--fdr needs --diff")
    if a.diff and a.ct_snp != "no-action":
        ap.error("--diff needs the C/T-SNP mode off")
    rng = np.random.default_rng(1)
    lens = np.array([int(x * a.genome) for x in (248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973, 145138636, 138394717, 133797422,
                                                135086622, 133275309, 114364328, 107043718, 101991189, 90338345, 83257441, 80373285, 58617616, 64444167,
                                                46709983, 50818468, 156040895, 57227415)], np.uint64)
    m = MR.Meth.from_lengths(lens, rm_dup=True)
    L, h = m.L, m.h   # the timed regions below that hold one library call and no fetch make that call directly
    if a.ct_snp != "no-action":
        m.set_ct_snp(a.ct_snp)
    if a.nonconv_filter:
        m.set_nonconv(a.nonconv_filter)
    if a.read_stats:
        m.set_read_stats()
    if a.pdr:
        m.set_pdr(a.pdr_min_cpg)
    letters = np.frombuffer(b"ACGT", np.uint8)
    chunks = []
    for c, n in enumerate(lens.tolist()):
        s = letters[rng.integers(0, 4, n, dtype=np.uint8)]
        m.set_reference(c, s.tobytes())   # (the array itself would do; the copy is kept as every earlier figure in profiles/ was taken with it)
        if c < 2:
            chunks.append(s)
    extra = {}
    if a.epi:  # after the reference is whole: the first call that needs the index builds it
        m.set_epi()
        t5, n_cpg = time.perf_counter(), 0
        for c in range(len(lens)):
            n_cpg += m.n_cpg(c)
        extra.update(cpg_index_build_s=round(time.perf_counter() - t5, 3), n_cpg=n_cpg)
    n, ln = a.aln, a.len
    # alignments on the first two chromosomes only need their letters on the host; positions are uniform there
    chr_ = rng.integers(0, 2, n).astype(np.uint32)
    pos = (rng.random(n) * (np.array([len(chunks[0]), len(chunks[1])])[chr_] - ln - 1)).astype(np.int64)
    strand = rng.integers(0, 4, n).astype(np.uint8)
    seq = np.empty((n, ln), np.uint8)
    for c in (0, 1):
        sel = np.nonzero(chr_ == c)[0]
        idx = pos[sel, None] + np.arange(ln)[None, :]
        seq[sel] = chunks[c][idx]
    conv = rng.random((n, ln)) < 0.7  # unmethylated fraction
    plus = (strand & 1) == 0
    seq_b = seq.copy() if a.diff else None   # sample B: the same reads, converted under another seed
    seq[plus[:, None] & (seq == ord("C")) & conv] = ord("T")
    seq[(~plus)[:, None] & (seq == ord("G")) & conv] = ord("A")
    ins = np.zeros(n, np.int32); cut = np.full(n, -1, np.int64)
    off = (np.arange(n + 1, dtype=np.uint64) * ln)
    mb = None
    if a.diff:
        conv = np.random.default_rng(2).random((n, ln)) < 0.5
        seq_b[plus[:, None] & (seq_b == ord("C")) & conv] = ord("T")
        seq_b[(~plus)[:, None] & (seq_b == ord("G")) & conv] = ord("A")
        mb = MR.Meth.from_lengths(lens, rm_dup=True)
        for c in (0, 1):   # the alignments lie on the first two chromosomes: B's pile-up reads no other letters, and the diff calls read A's
            mb.set_reference(c, chunks[c])
        mb.add_arrays(n, chr_, pos, strand, ins, cut, seq_b, off, 2)
        del seq_b, conv
    m.add_arrays(min(n, 1 << 20), chr_, pos, strand, ins, cut, seq, off, 2)
    t0 = time.perf_counter()
    m.add_arrays(n, chr_, pos, strand, ins, cut, seq, off, 2)   # every array has its type already: passed as it is
    dt = time.perf_counter() - t0
    t1 = time.perf_counter()
    rows = cov = 0
    for c in range(len(lens)):
        nr, cv, sd = C.c_uint32(), C.c_uint64(), C.c_uint64()
        B._check(L.bsx_meth_report_chr(h, c, 1, 1, C.byref(nr), C.byref(cv), C.byref(sd)))
        rows += nr.value; cov += cv.value
    dt_rep = time.perf_counter() - t1
    if a.nonconv_filter:
        extra.update(nonconv_filter=a.nonconv_filter, dropped=m.nonconv_dropped())
    if a.read_stats:
        extra["read_stats_totals"] = dict(zip(("reads", "cg_over", "ch_calls", "ch_meth"), m.read_stats()[2]))
    if a.pdr:
        t4, pdr_rows = time.perf_counter(), 0
        for c in range(len(lens)):
            nr = C.c_uint32()
            B._check(L.bsx_meth_pdr_report_chr(h, c, 1, C.byref(nr)))
            pdr_rows += nr.value
        extra.update(pdr_min_cpg=a.pdr_min_cpg, pdr_rows=pdr_rows, pdr_report_s_all_chromosomes=round(time.perf_counter() - t4, 3))
    if a.epi:
        t6, epi_rows = time.perf_counter(), 0
        for c in range(len(lens)):
            nr = C.c_uint32()
            B._check(L.bsx_meth_epi_report_chr(h, c, 1, C.byref(nr)))
            epi_rows += nr.value
        extra.update(epi_rows=epi_rows, epi_report_s_all_chromosomes=round(time.perf_counter() - t6, 3))
    if a.diff:
        t7, diff_rows = time.perf_counter(), 0
        for c in range(len(lens)):
            nr = C.c_uint32()
            B._check(L.bsx_meth_diff_report_chr(h, mb.h, c, 1, a.diff_delta, C.byref(nr)))
            diff_rows += nr.value
        extra.update(diff_delta_permille=a.diff_delta, diff_rows=diff_rows, diff_report_s_all_chromosomes=round(time.perf_counter() - t7, 3))
    if a.fdr:
        t9, n_all, n_dmr = time.perf_counter(), C.c_uint64(), C.c_uint32()
        B._check(L.bsx_meth_diff_report_all(h, mb.h, 1, C.byref(n_all)))
        t10 = time.perf_counter()
        B._check(L.bsx_meth_diff_dmrs(h, mb.h, 1, C.byref(C.c_double(a.dmr_max_q)), a.diff_delta, 300, 3, C.byref(n_dmr)))
        extra.update(store_rows=n_all.value, diff_report_all_s=round(t10 - t9, 3), dmr_max_q=a.dmr_max_q, dmrs=n_dmr.value, diff_dmrs_s=round(time.perf_counter() - t10, 3))
    for width in [int(x) for x in a.wig_bin.split(",") if x]:
        out = np.zeros((int(lens.max()) // width + 1, 5), np.uint64)
        nb, took = C.c_uint64(), []
        for _ in range(a.repeat):
            sites, t2 = 0, time.perf_counter()
            for c in range(len(lens)):
                B._check(L.bsx_meth_bins(h, c, width, 1, len(out), out.ctypes.data, C.byref(nb)))
                sites += int(out[:nb.value, 0].sum())
            took.append(round(time.perf_counter() - t2, 3))
        extra.setdefault("bins_s_all_chromosomes", []).append({"wig_bin": width, "s": took, "sites": sites})
    for spec in [x for x in a.regions.split(";") if x]:
        n_iv, iv_len = (int(x) for x in spec.split(","))
        fits = np.nonzero(lens >= iv_len)[0]
        if len(fits) and fits[0] < 2:
            fits = fits[fits < 2]  # on the chromosomes that carry the alignments, where one of them is long enough
        ic = fits[rng.integers(0, len(fits), n_iv)].astype(np.uint32)
        start = (rng.random(n_iv) * (lens[ic] - iv_len + 1)).astype(np.uint32)
        end = (start + iv_len).astype(np.uint32)
        sums, took = np.zeros((n_iv, 5), np.uint64), []
        for _ in range(a.repeat):
            t3 = time.perf_counter()
            B._check(L.bsx_meth_regions(h, n_iv, ic.ctypes.data, start.ctypes.data, end.ctypes.data, 1, sums.ctypes.data))
            took.append(round(time.perf_counter() - t3, 3))
        extra.setdefault("regions_s", []).append({"intervals": n_iv, "len": iv_len, "s": took, "sites": int(sums[:, 0].sum())})
        if a.diff:
            p, took = np.zeros(n_iv, np.float64), []
            for _ in range(a.repeat):
                t8 = time.perf_counter()
                B._check(L.bsx_meth_diff_regions(h, mb.h, n_iv, ic.ctypes.data, start.ctypes.data, end.ctypes.data, 1, sums.ctypes.data, p.ctypes.data))
                took.append(round(time.perf_counter() - t8, 3))
            extra.setdefault("diff_regions_s", []).append({"intervals": n_iv, "len": iv_len, "s": took, "common_sites": int(sums[:, 0].sum())})
    if mb is not None:
        mb.close()
    m.close()
    print(json.dumps(dict({"alignments": n, "read_len": ln, "ct_snp": a.ct_snp, "add_s_incl_pcie": round(dt, 3), "alignments_per_s_incl_pcie": round(n / dt),
                           "report_s_all_chromosomes": round(dt_rep, 3), "rows": rows, "covered": cov, "genome_bp": int(lens.sum())}, **extra)))


if __name__ == "__main__":
    main()
