#!/usr/bin/env python3
"""methratio — methylation ratios from BSMAP alignments, pile-up on the GPU.

Host-side mirror of the reference's methratio.py (same option letters, same input formats, same table, same summary
line).  This file keeps the option surface; the FASTA and the mapping files are parsed by host threads inside
libbsx.so (bsx_meth_create_from_fasta, bsx_meth_add_file), the per-alignment work — duplicate removal, fill-in trimming, the counter updates under
every reference C/G — and the selection of table rows run in HIP kernels, and the table is formatted by host threads
(bsx_meth_write_table), all behind the C ABI of include/bsx.h.  There is no CPU
fallback: without the library and a gfx950 device this fails.

    python -m bsmap_amd.methratio -o out.txt -d genome.fa [options] alignments.bsp|.sam [...]

Differences from the reference: SAM and BAM files are read directly (numeric flags: 0x4 = 'u', 0x100 = 's', 0x2 = 'P' of
`samtools view -X`; BGZF through zlib), no samtools is spawned and `-s` is accepted and ignored.  Extensions: `--mbias=FILE`
writes the M-bias table (methylated / all calls per sequencing cycle, strand and cytosine context, tallied by the pile-up
kernel), `--trim-5p=N` / `--trim-3p=N` ignore the calls of the first / last N cycles of every read.  From later BSMAP releases:
`-i/--ct-snp {no-action,correct,skip}` counts, in the same pile-up, what the reads of the other reference strand show over every C (G: intact, A: a C->T
SNP) and corrects the depth by that share or skips the position, with their 12-column table (default here: no-action, the table above); `-x/--context
CG,CHG,CHH` lists the cytosines of those contexts only; `-w/--wig FILE` with `-b/--wig-bin N` (default 25) writes a wiggle track of the pooled
methylation ratio per bin of N nt.  Extension: `--regions BED --region-out FILE` writes one pooled ratio per BED interval (promoters, CpG islands, capture
targets).  Both are sums of the counters on the GPU (bsx_meth_bins, bsx_meth_regions) under the table's row rule (-m, -x, -i; after -g), not a pass
over the table's text.  Per-read extensions (a call = a letter that enters a cytosine's depth, counted per alignment line by the k_meth_reads kernel
ahead of the pile-up): `--nonconv-filter N` drops every read with N or more methylated non-CpG calls (Bismark's filter_non_conversion) from every output and
from "valid mappings"; `--read-stats FILE` writes the histogram of reads by their CpG calls / methylated CpG calls and by their methylated non-CpG calls, the
curve N is read off (it does not depend on N); `--pdr FILE` writes, per CpG position, the reads with at least `--pdr-min-cpg K` (default 4) CpG calls that
cover it and how many of them are discordant (neither all methylated nor all unmethylated): the proportion of discordant reads of Landau et al. 2014, for
positions with at least `--pdr-min-reads R` (default 1) such reads, after the `-g` fold.  `--epi FILE` (the k_meth_epi kernel over a CpG index
of the reference) writes, per window of four neighbouring reference CpGs, how many reads show each of the sixteen methylation patterns: a read counts for a
window when it makes a CpG call at all four, and the `--nonconv-filter`, the cycle trims, `-r` and `-t` apply to it as to every call, while `-g`, `-x`, `-i`
and `-m` do not touch it; each row carries the epipolymorphism (Landan et al. 2012) and the methylation entropy (Xie et al. 2011) of its sixteen counts,
for windows with at least `--epi-min-reads R` (default 1) reads."""
import ctypes as C
import sys
import time

import numpy as np

from . import lib, _check

RS_CG, RS_CH = 32, 64  # BSX_RS_CG_MAX + 1, BSX_RS_CH_MAX + 1 of include/bsx.h: bsx_meth_read_stats_fetch fills cg[RS_CG][RS_CG], ch[RS_CH], totals[4]
MBIAS_CYCLES = 1024  # BSX_MBIAS_CYCLES of include/bsx.h: bsx_meth_mbias_fetch fills [4][4][MBIAS_CYCLES][2] uint64
MBIAS_STRANDS = ("++", "-+", "+-", "--")
MBIAS_CONTEXTS = ("CG", "CHG", "CHH", "CN")
CT_SNP_MODES = ("no-action", "correct", "skip")  # bsx_meth_set_ct_snp modes 0, 1, 2
CONTEXT_BITS = {"CG": 1, "CHG": 2, "CHH": 4}      # bsx_meth_set_contexts

def _bind():
    L = lib()
    if getattr(L, "_meth_bound", False):
        return L
    vp, u32, i32, u64 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64
    L.bsx_meth_create.argtypes = [u32, vp, i32, i32, C.POINTER(vp)]
    L.bsx_meth_destroy.argtypes = [vp]; L.bsx_meth_destroy.restype = None
    L.bsx_meth_set_reference.argtypes = [vp, u32, C.c_char_p]
    L.bsx_meth_add.argtypes = [vp, u32, vp, vp, vp, vp, vp, vp, vp, u32]
    L.bsx_meth_combine_cpg.argtypes = [vp]
    L.bsx_meth_valid_mappings.argtypes = [vp, vp]
    L.bsx_meth_report_chr.argtypes = [vp, u32, u32, i32, vp, vp, vp]
    L.bsx_meth_fetch_rows.argtypes = [vp, vp, vp, vp]
    L.bsx_meth_create_from_fasta.argtypes = [C.c_char_p, C.c_char_p, i32, i32, C.POINTER(vp)]
    L.bsx_meth_add_file.argtypes = [vp, C.c_char_p, i32, vp, i32, i32, u32, vp]
    L.bsx_meth_write_table.argtypes = [vp, C.c_char_p, u32, vp, vp, u32, i32, vp, vp]
    L.bsx_meth_set_cycle_trim.argtypes = [vp, u32, u32]
    L.bsx_meth_set_mbias.argtypes = [vp, i32]
    L.bsx_meth_mbias_fetch.argtypes = [vp, vp, vp]
    L.bsx_meth_write_mbias.argtypes = [vp, C.c_char_p]
    L.bsx_meth_set_ct_snp.argtypes = [vp, i32]
    L.bsx_meth_set_contexts.argtypes = [vp, u32]
    L.bsx_meth_fetch_rows_snp.argtypes = [vp, vp, vp]
    L.bsx_meth_region_tile.argtypes = []; L.bsx_meth_region_tile.restype = u32
    L.bsx_meth_regions.argtypes = [vp, u32, vp, vp, vp, u32, vp]
    L.bsx_meth_bins.argtypes = [vp, u32, u32, u32, u64, vp, vp]
    L.bsx_meth_write_regions.argtypes = [vp, C.c_char_p, C.c_char_p, u32, vp, vp]
    L.bsx_meth_write_wig.argtypes = [vp, C.c_char_p, u32, u32]
    L.bsx_meth_set_nonconv.argtypes = [vp, u32]
    L.bsx_meth_nonconv_dropped.argtypes = [vp, vp]
    L.bsx_meth_set_read_stats.argtypes = [vp, i32]
    L.bsx_meth_read_stats_fetch.argtypes = [vp, vp, vp, vp]
    L.bsx_meth_write_read_stats.argtypes = [vp, C.c_char_p]
    L.bsx_meth_set_pdr.argtypes = [vp, u32]
    L.bsx_meth_pdr_report_chr.argtypes = [vp, u32, u32, vp]
    L.bsx_meth_pdr_fetch_rows.argtypes = [vp, vp, vp, vp]
    L.bsx_meth_write_pdr.argtypes = [vp, C.c_char_p, u32, vp]
    L.bsx_meth_set_epi.argtypes = [vp, i32]
    L.bsx_meth_n_cpg.argtypes = [vp, u32, vp]
    L.bsx_meth_epi_report_chr.argtypes = [vp, u32, u32, vp]
    L.bsx_meth_epi_fetch_rows.argtypes = [vp, vp, vp]
    L.bsx_meth_write_epi.argtypes = [vp, C.c_char_p, u32, vp]
    L._meth_bound = True
    return L


def mbias_fetch(L, h):
    """the M-bias cells of a handle as uint64 [strand][context][cycle][unmethylated, methylated] and the count of calls beyond the last cycle"""
    cells = np.zeros((4, 4, MBIAS_CYCLES, 2), np.uint64)
    over = C.c_uint64()
    _check(L.bsx_meth_mbias_fetch(h, cells.ctypes.data, C.byref(over)))
    return cells, over.value


def read_stats_fetch(L, h):
    """the read histogram of a handle: cg[n_cg][m_cg] and ch[min(m_ch, 63)] as uint64, and the totals (reads, cg_over, ch_calls, ch_meth)"""
    cg, ch, tot = np.zeros((RS_CG, RS_CG), np.uint64), np.zeros(RS_CH, np.uint64), np.zeros(4, np.uint64)
    _check(L.bsx_meth_read_stats_fetch(h, cg.ctypes.data, ch.ctypes.data, tot.ctypes.data))
    return cg, ch, tuple(int(x) for x in tot)


def epi_fetch(L, h, chr, min_reads=1):
    """the epiallele rows of one sequence with at least min_reads reads: pos0 as uint32 [rows][4] (the 0-based positions of the four Cs) and counts as
    uint32 [rows][16] (by pattern: bit j set = CpG j of the window methylated)"""
    nr = C.c_uint32()
    _check(L.bsx_meth_epi_report_chr(h, chr, min_reads, C.byref(nr)))
    pos0, counts = np.zeros((nr.value, 4), np.uint32), np.zeros((nr.value, 16), np.uint32)
    _check(L.bsx_meth_epi_fetch_rows(h, pos0.ctypes.data, counts.ctypes.data))
    return pos0, counts


def load_reference(path, chroms):
    """methratio.py:67-77"""
    ref, cr, seq = {}, "", []
    with open(path) as f:
        for line in f:
            if line[0] == ">":
                if cr and (not chroms or cr in chroms):
                    ref[cr] = "".join(seq).upper()
                cr, seq = line[1:-1].split()[0], []
            else:
                seq.append(line.strip())
    if not chroms or cr in chroms:
        ref[cr] = "".join(seq).upper()
    return ref


def run(reffile, infiles, outfile, chroms=None, unique=False, pair=False, meth0=False, rm_dup=False, trim_fillin=2, combine_CpG=False,
        min_depth=1, device=0, quiet=True, mbias=None, trim5=0, trim3=0, ct_snp="no-action", context=None, wig=None, wig_bin=25, regions=None, region_out=None,
        nonconv_filter=0, read_stats=None, pdr=None, pdr_min_cpg=None, pdr_min_reads=None, epi=None, epi_min_reads=None):
    """returns the summary line the reference prints on stdout; ct_snp: one of CT_SNP_MODES, context: names of CONTEXT_BITS to list (None: all);
    wig: wiggle file of the pooled ratio per bin of wig_bin nt; regions / region_out: BED file in, one pooled ratio per interval out;
    nonconv_filter: drop reads with that many methylated non-CpG calls (0: off); read_stats: file of the read histogram; pdr: file of the proportion of
    discordant reads, over reads with pdr_min_cpg (default 4) CpG calls, for positions with pdr_min_reads (default 1) of them; epi: file of the
    epiallele patterns per window of four CpGs, for windows with epi_min_reads (default 1) reads"""
    if nonconv_filter < 0:
        raise ValueError("nonconv_filter cannot be negative")
    if pdr is None and (pdr_min_cpg is not None or pdr_min_reads is not None):
        raise ValueError("pdr_min_cpg and pdr_min_reads need pdr")
    pdr_min_cpg = 4 if pdr_min_cpg is None else pdr_min_cpg
    pdr_min_reads = 1 if pdr_min_reads is None else pdr_min_reads
    if pdr_min_cpg < 1 or pdr_min_reads < 1:
        raise ValueError("pdr_min_cpg and pdr_min_reads are at least 1")
    if epi is None and epi_min_reads is not None:
        raise ValueError("epi_min_reads needs epi")
    epi_min_reads = 1 if epi_min_reads is None else epi_min_reads
    if epi_min_reads < 1:
        raise ValueError("epi_min_reads is at least 1")
    if wig_bin < 1:
        raise ValueError("wig_bin must be at least 1")
    if (regions is None) != (region_out is None):
        raise ValueError("regions and region_out go together")
    if ct_snp not in CT_SNP_MODES:
        raise ValueError("ct_snp must be one of %s" % ", ".join(CT_SNP_MODES))
    if context is not None and (not context or any(x not in CONTEXT_BITS for x in context)):
        raise ValueError("context must be a non-empty subset of %s" % ", ".join(CONTEXT_BITS))
    def disp(txt):
        if not quiet:
            sys.stderr.write("@ %s: %s\n" % (time.asctime(), txt))

    L = _bind()
    disp("reading reference %s ..." % reffile)
    h = C.c_void_p()
    _check(L.bsx_meth_create_from_fasta(reffile.encode(), ",".join(chroms).encode() if chroms else None, 1 if rm_dup else 0, device, C.byref(h)))
    try:
        if mbias:
            _check(L.bsx_meth_set_mbias(h, 1))
        if trim5 or trim3:
            _check(L.bsx_meth_set_cycle_trim(h, trim5, trim3))
        if ct_snp != "no-action":
            _check(L.bsx_meth_set_ct_snp(h, CT_SNP_MODES.index(ct_snp)))
        if context is not None:
            _check(L.bsx_meth_set_contexts(h, sum(CONTEXT_BITS[x] for x in set(context))))
        if nonconv_filter:
            _check(L.bsx_meth_set_nonconv(h, nonconv_filter))
        if read_stats is not None:
            _check(L.bsx_meth_set_read_stats(h, 1))
        if pdr is not None:
            _check(L.bsx_meth_set_pdr(h, pdr_min_cpg))
        if epi is not None:
            _check(L.bsx_meth_set_epi(h, 1))
        for infile in infiles:
            disp("reading %s ..." % infile)
            ext = infile[-4:].upper()
            nl = C.c_uint64()
            _check(L.bsx_meth_add_file(h, infile.encode(), 2 if ext == ".BAM" else 1 if ext == ".SAM" else 0, None, 1 if unique else 0, 1 if pair else 0, max(0, trim_fillin), C.byref(nl)))
        if mbias:
            disp("writing %s ..." % mbias)
            _check(L.bsx_meth_write_mbias(h, mbias.encode()))
        if nonconv_filter:
            ndropped = C.c_uint64()
            _check(L.bsx_meth_nonconv_dropped(h, C.byref(ndropped)))
            disp("%d reads with %d or more methylated non-CpG calls dropped" % (ndropped.value, nonconv_filter))
        if read_stats is not None:
            disp("writing %s ..." % read_stats)
            _check(L.bsx_meth_write_read_stats(h, read_stats.encode()))
        if combine_CpG:
            disp("combining CpG methylation from both strands ...")
            _check(L.bsx_meth_combine_cpg(h))
        disp("writing %s ..." % outfile)
        nc, nd, nmap = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(L.bsx_meth_write_table(h, outfile.encode(), 0, None, None, min_depth, 1 if meth0 else 0, C.byref(nc), C.byref(nd)))
        _check(L.bsx_meth_valid_mappings(h, C.byref(nmap)))
        if pdr is not None:
            disp("writing %s ..." % pdr)
            _check(L.bsx_meth_write_pdr(h, pdr.encode(), pdr_min_reads, None))
        if epi is not None:
            disp("writing %s ..." % epi)
            _check(L.bsx_meth_write_epi(h, epi.encode(), epi_min_reads, None))
        if wig is not None:
            disp("writing %s ..." % wig)
            _check(L.bsx_meth_write_wig(h, wig.encode(), wig_bin, min_depth))
        if regions is not None:
            disp("writing %s ..." % region_out)
            nw, ndrop = C.c_uint64(), C.c_uint64()
            _check(L.bsx_meth_write_regions(h, regions.encode(), region_out.encode(), min_depth, C.byref(nw), C.byref(ndrop)))
            disp("%d intervals of %s written, %d on sequences that are not loaded dropped" % (nw.value, regions, ndrop.value))
        disp("done.")
        # (with nothing covered the reference dies here on a division by zero; that is reported instead)
        if nc.value == 0:
            return "total %d valid mappings, 0 covered cytosines.\n" % nmap.value
        return "total %d valid mappings, %d covered cytosines, average coverage: %.2f fold.\n" % (nmap.value, nc.value, float(nd.value) / nc.value)
    finally:
        L.bsx_meth_destroy(h)


def build_parser():
    """the command line with the reference's option letters (methratio.py:3-17) and the extensions"""
    import argparse
    class Parser(argparse.ArgumentParser):
        def parse_args(self, args=None, namespace=None):
            o = super().parse_args(args, namespace)
            if o.pdr is None and o.pdr_only:
                self.error("%s needs --pdr" % ", ".join(o.pdr_only))
            if o.epi is None and o.epi_min_reads is not None:
                self.error("--epi-min-reads needs --epi")
            return o
    class PdrOnly(argparse.Action):  # stores the value and remembers that the option was given
        def __call__(self, parser, namespace, values, option_string=None):
            setattr(namespace, self.dest, values)
            namespace.pdr_only = namespace.pdr_only + [option_string]
    ap = Parser(prog="methratio", description="methylation ratios from BSMAP mapping files (BSP, SAM or BAM), pile-up on the GPU")
    ap.add_argument("-o", "--out", dest="outfile", required=True, help="table to write")
    ap.add_argument("-d", "--ref", dest="reffile", required=True, help="reference FASTA the reads were mapped to")
    ap.add_argument("-c", "--chr", dest="chroms", default="", help="comma-separated sequence names to keep (default: every sequence)")
    ap.add_argument("-s", "--sam-path", dest="sam_path", default="", help="ignored: SAM files are parsed directly, samtools is not needed")
    ap.add_argument("-u", "--unique", action="store_true", help="use uniquely mapped reads / pairs only")
    ap.add_argument("-p", "--pair", action="store_true", help="use properly paired mappings only")
    ap.add_argument("-z", "--zero-meth", dest="meth0", action="store_true", help="also list covered cytosines without a methylated read")
    ap.add_argument("-q", "--quiet", action="store_true", help="no progress lines on stderr")
    ap.add_argument("-r", "--remove-duplicate", dest="rm_dup", action="store_true", help="keep the first read per fragment end and direction")
    ap.add_argument("-t", "--trim-fillin", dest="trim_fillin", type=int, default=2, help="end-repair nucleotides to ignore at fragment ends (default 2)")
    ap.add_argument("-g", "--combine-CpG", dest="combine_CpG", action="store_true", help="add the counts of the G of each CpG to its C")
    ap.add_argument("-m", "--min-depth", dest="min_depth", type=int, default=1, help="lowest depth a listed cytosine must have (default 1)")
    ap.add_argument("-G", "--gpu", dest="device", type=int, default=0, help="GPU ordinal (extension)")
    def cycles(txt):
        n = int(txt)
        if n < 0:
            raise argparse.ArgumentTypeError("a number of cycles cannot be negative")
        return n
    ap.add_argument("--mbias", dest="mbias", default=None, metavar="FILE", help="write the M-bias table: methylated / all calls per read cycle, strand and context (extension)")
    ap.add_argument("--trim-5p", dest="trim5", type=cycles, default=0, metavar="N", help="ignore the calls of the first N sequencing cycles of every read (extension, default 0)")
    ap.add_argument("--trim-3p", dest="trim3", type=cycles, default=0, metavar="N", help="ignore the calls of the last N sequencing cycles of every read (extension, default 0)")
    def contexts(txt):
        names = txt.split(",")
        if any(x not in CONTEXT_BITS for x in names):
            raise argparse.ArgumentTypeError("a comma-separated list of CG, CHG, CHH is expected")
        return names
    ap.add_argument("-i", "--ct-snp", dest="ct_snp", choices=CT_SNP_MODES, default="no-action",
                    help="C/T SNPs, told from unmethylated C by the reads of the other strand: correct the depth, skip the position, or no-action (default)")
    ap.add_argument("-x", "--context", dest="context", type=contexts, default=None, metavar="CG,CHG,CHH", help="list cytosines of these contexts only (default: all)")
    def bin_width(txt):
        n = int(txt)
        if n < 1:
            raise argparse.ArgumentTypeError("a bin is at least 1 nt wide")
        return n
    ap.add_argument("-w", "--wig", dest="wig", default=None, metavar="FILE", help="write a wiggle track of the pooled methylation ratio per bin")
    ap.add_argument("-b", "--wig-bin", dest="wig_bin", type=bin_width, default=25, metavar="N", help="bin width of the wiggle track in nt (default 25)")
    ap.add_argument("--regions", dest="regions", default=None, metavar="BED", help="intervals (BED: name, start, end, optional label) to pool the methylation over (extension)")
    ap.add_argument("--region-out", dest="region_out", default=None, metavar="FILE", help="table to write for --regions: one pooled ratio per interval, in the BED file's order")
    def at_least(lowest, what):
        def parse(txt):
            n = int(txt)
            if n < lowest:
                raise argparse.ArgumentTypeError("%s is at least %d" % (what, lowest))
            return n
        return parse
    ap.add_argument("--nonconv-filter", dest="nonconv_filter", type=at_least(0, "the threshold"), default=0, metavar="N",
                    help="drop reads with N or more methylated non-CpG calls: reads the bisulfite conversion missed (extension, default 0: off)")
    ap.add_argument("--read-stats", dest="read_stats", default=None, metavar="FILE",
                    help="write the histogram of reads by CpG calls / methylated CpG calls and by methylated non-CpG calls (extension)")
    ap.add_argument("--pdr", dest="pdr", default=None, metavar="FILE", help="write the proportion of discordant reads per CpG position (extension)")
    ap.set_defaults(pdr_only=[])
    ap.add_argument("--pdr-min-cpg", dest="pdr_min_cpg", action=PdrOnly, type=at_least(1, "the number of CpG calls"), default=4, metavar="K",
                    help="CpG calls a read needs to count for --pdr (default 4)")
    ap.add_argument("--pdr-min-reads", dest="pdr_min_reads", action=PdrOnly, type=at_least(1, "the number of reads"), default=1, metavar="R",
                    help="such reads a position needs for a row of --pdr (default 1)")
    ap.add_argument("--epi", dest="epi", default=None, metavar="FILE",
                    help="write the epiallele table: reads per methylation pattern of every four neighbouring CpGs, with epipolymorphism and entropy (extension)")
    ap.add_argument("--epi-min-reads", dest="epi_min_reads", type=at_least(1, "the number of reads"), default=None, metavar="R",
                    help="reads a window needs for a row of --epi (default 1)")
    ap.add_argument("infiles", nargs="+", help="mapping files written by bsmap: *.sam / *.bam by their format, anything else as BSP")
    return ap


def main(argv=None):
    """the command line: parses argv (default sys.argv[1:]) and prints run()'s summary line"""
    o = build_parser().parse_args(argv)
    sys.stdout.write(run(o.reffile, o.infiles, o.outfile, chroms=o.chroms.split(",") if o.chroms else None, unique=o.unique, pair=o.pair, meth0=o.meth0,
                         rm_dup=o.rm_dup, trim_fillin=o.trim_fillin, combine_CpG=o.combine_CpG, min_depth=o.min_depth, device=o.device, quiet=o.quiet,
                         mbias=o.mbias, trim5=o.trim5, trim3=o.trim3, ct_snp=o.ct_snp, context=o.context, wig=o.wig, wig_bin=o.wig_bin,
                         regions=o.regions, region_out=o.region_out, nonconv_filter=o.nonconv_filter, read_stats=o.read_stats, pdr=o.pdr,
                         pdr_min_cpg=o.pdr_min_cpg if o.pdr is not None else None, pdr_min_reads=o.pdr_min_reads if o.pdr is not None else None,
                         epi=o.epi, epi_min_reads=o.epi_min_reads))


if __name__ == "__main__":
    main()
