#!/usr/bin/env python3
"""methdiff — differentially methylated cytosines and regions of two samples, both pile-ups and the test on the GPU.

    python -m bsmap_amd.methdiff -d genome.fa -o dml.txt --a ctrl1.sam [ctrl2.bam ..] --b case1.sam [..]
        [--min-delta 0.25] [--max-p 0.01] [--regions BED --region-out FILE] [--bin N --bin-out FILE]
        [--fdr] [--max-q 0.05] [--dmr-out FILE [--dmr-max-q 0.05] [--dmr-max-gap 300] [--dmr-min-sites 3]]

The mapping files of `--a` are pooled into one pile-up and those of `--b` into another (two bsx_meth handles side by side in HBM), under the pile-up
options of methratio (-c -u -p -r -t -g -m -x -G --trim-5p --trim-3p --nonconv-filter: the same meanings, applied to both samples; the C/T-SNP modes of
-i are not offered).  A common site is a cytosine that the row rule (-m, -x) lists in both samples.  `-o` gets one row per common site whose
methylation ratios differ by `--min-delta` or more (default 0: every common site), with both samples' counts and ratios, delta = ratio_b - ratio_a and
the p-value of the two-sided Fisher exact test of the 2 x 2 table of its counts (k_meth_fisher), and with `--max-p` only the rows with p at or below it.
`--regions BED --region-out FILE` writes the same for the pooled counts of every BED interval, `--bin N --bin-out FILE` for every bin of N nt that
holds a common site.

`--fdr` adds a column q to `-o` and `--region-out`: the Benjamini-Hochberg q-value of the row.  For `-o` the family is every common site of
every loaded sequence, whatever `--min-delta`, `--max-p` and `--max-q` leave out of the file; for `--region-out` it is the file's intervals that hold a
common site.  `--max-q Q` implies `--fdr` and lists only the cytosines with q at or below Q.  The bin file has no q column (it is written in pieces).
`--dmr-out FILE` writes de novo differentially methylated regions: maximal runs of cytosines with q at or below `--dmr-max-q` (default 0.05) and a
difference of `--min-delta` or more in one direction, each at most `--dmr-max-gap` nt (default 300) behind the one before, with at least
`--dmr-min-sites` of them (default 3); a row has the span, that number, and the pooled counts, ratios, delta and Fisher p of ALL common cytosines of the
span: that p describes the region and is not a corrected value.  The three defaults are conventions of the field, not measurements.

    python -m bsmap_amd.methdiff -d genome.fa -o dml.txt --a ctrl.bam --b case.bam --min-delta 0.25 --max-q 0.05 --dmr-out dmr.txt

There is no CPU fallback: without the library and a gfx950 device this fails."""
import sys
import time

from .methratio import CONTEXT_BITS, Meth


def run(reffile, a_files, b_files, outfile, chroms=None, unique=False, pair=False, rm_dup=False, trim_fillin=2, combine_CpG=False, min_depth=1, device=0,
        quiet=True, trim5=0, trim3=0, context=None, nonconv_filter=0, min_delta=0.0, max_p=None, regions=None, region_out=None, bin=None, bin_out=None,
        fdr=False, max_q=None, dmr_out=None, dmr_max_q=None, dmr_max_gap=None, dmr_min_sites=None):
    """returns the summary line; min_delta: 0 .. 1, the least |ratio_b - ratio_a| of a row; max_p: rows of the position file with p above it are left
    out (None: none); regions / region_out: BED file in, one row per interval out; bin / bin_out: bin width in nt, one row per bin with a common site out;
    fdr: a q column in outfile and region_out; max_q: implies fdr, rows of the position file with q above it are left out; dmr_out: the DMR file, with
    dmr_max_q (None: 0.05), dmr_max_gap (None: 300) and dmr_min_sites (None: 3), which need it"""
    if not a_files or not b_files:
        raise ValueError("both samples need at least one mapping file")
    if not (isinstance(min_delta, (int, float)) and 0.0 <= min_delta <= 1.0):   # (a NaN fails both comparisons)
        raise ValueError("min_delta must be within 0 .. 1")
    permille = int(round(min_delta * 1000))
    if max_p is not None and not (0.0 <= max_p <= 1.0):
        raise ValueError("max_p must be within 0 .. 1")
    if (regions is None) != (region_out is None):
        raise ValueError("regions and region_out go together")
    if (bin is None) != (bin_out is None):
        raise ValueError("bin and bin_out go together")
    if bin is not None and bin < 1:
        raise ValueError("bin must be at least 1")
    number = lambda x: isinstance(x, (int, float))
    if max_q is not None and not (number(max_q) and 0.0 <= max_q <= 1.0):
        raise ValueError("max_q must be within 0 .. 1")
    if dmr_out is None and not (dmr_max_q is None and dmr_max_gap is None and dmr_min_sites is None):
        raise ValueError("dmr_max_q, dmr_max_gap and dmr_min_sites need dmr_out")
    dmr_max_q, dmr_max_gap, dmr_min_sites = (d if x is None else x for x, d in ((dmr_max_q, 0.05), (dmr_max_gap, 300), (dmr_min_sites, 3)))
    if not (number(dmr_max_q) and 0.0 <= dmr_max_q <= 1.0):
        raise ValueError("dmr_max_q must be within 0 .. 1")
    if not (isinstance(dmr_max_gap, int) and isinstance(dmr_min_sites, int) and 0 <= dmr_max_gap <= 0xFFFFFFFF and 1 <= dmr_min_sites <= 0xFFFFFFFF):
        raise ValueError("dmr_max_gap cannot be negative and dmr_min_sites must be at least 1")
    fdr = bool(fdr) or max_q is not None
    if min_depth < 0 or nonconv_filter < 0 or trim5 < 0 or trim3 < 0:
        raise ValueError("min_depth, nonconv_filter, trim5 and trim3 cannot be negative")
    if context is not None and (not context or any(x not in CONTEXT_BITS for x in context)):
        raise ValueError("context must be a non-empty subset of %s" % ", ".join(CONTEXT_BITS))

    def disp(txt):
        if not quiet:
            sys.stderr.write("@ %s: %s\n" % (time.asctime(), txt))

    def pile_up(m, files):
        if trim5 or trim3:
            m.set_cycle_trim(trim5, trim3)
        if context is not None:
            m.set_contexts(sum(CONTEXT_BITS[x] for x in set(context)))
        if nonconv_filter:
            m.set_nonconv(nonconv_filter)
        for f in files:
            disp("reading %s ..." % f)
            m.add_file(f, unique, pair, max(0, trim_fillin))
        if combine_CpG:
            m.combine_cpg()
        return m.valid_mappings()

    disp("reading reference %s ..." % reffile)
    with Meth.from_fasta(reffile, chroms, rm_dup, device) as a, Meth.from_fasta(reffile, chroms, rm_dup, device) as b:
        n_a, n_b = pile_up(a, a_files), pile_up(b, b_files)
        n_chr = a.n_chr
        whole, _ = a.diff_regions(b, range(n_chr), [0] * n_chr, [0xFFFFFFFF] * n_chr, min_depth)   # clipped to every sequence's length
        disp("writing %s ..." % outfile)
        rows = a.write_diff(b, outfile, min_depth, permille, max_p, max_q, fdr)
        if regions is not None:
            disp("writing %s ..." % region_out)
            nw, ndrop = a.write_diff_regions(b, regions, region_out, min_depth, fdr)
            disp("%d intervals of %s written, %d on sequences that are not loaded dropped" % (nw, regions, ndrop))
        if bin is not None:
            disp("writing %s ..." % bin_out)
            a.write_diff_bins(b, bin_out, bin, min_depth)
        dmrs = ""
        if dmr_out is not None:
            disp("writing %s ..." % dmr_out)
            dmrs = ", %d DMRs written" % a.write_dmrs(b, dmr_out, dmr_max_q, permille, dmr_max_gap, dmr_min_sites, min_depth)
        disp("done.")
        return "total %d valid mappings in a, %d in b, %d common cytosines, %d rows written%s.\n" % (n_a, n_b, int(whole[:, 0].sum()), rows, dmrs)


def build_parser():
    import argparse

    def at_least(lowest, what):
        def parse(txt):
            n = int(txt)
            if n < lowest:
                raise argparse.ArgumentTypeError("%s is at least %d" % (what, lowest))
            return n
        return parse

    def fraction(txt):
        x = float(txt)
        if not 0.0 <= x <= 1.0:
            raise argparse.ArgumentTypeError("a value within 0 .. 1 is expected")
        return x

    def contexts(txt):
        names = txt.split(",")
        if any(x not in CONTEXT_BITS for x in names):
            raise argparse.ArgumentTypeError("a comma-separated list of CG, CHG, CHH is expected")
        return names

    class Parser(argparse.ArgumentParser):
        def parse_args(self, args=None, namespace=None):
            o = super().parse_args(args, namespace)
            if (o.regions is None) != (o.region_out is None):
                self.error("--regions and --region-out go together")
            if (o.bin is None) != (o.bin_out is None):
                self.error("--bin and --bin-out go together")
            if o.dmr_out is None and not (o.dmr_max_q is None and o.dmr_max_gap is None and o.dmr_min_sites is None):
                self.error("--dmr-max-q, --dmr-max-gap and --dmr-min-sites need --dmr-out")
            o.fdr = o.fdr or o.max_q is not None
            return o

    ap = Parser(prog="methdiff", description="differential methylation of two samples from BSMAP mapping files (BSP, SAM or BAM), on the GPU")
    ap.add_argument("-o", "--out", dest="outfile", required=True, help="position file to write: one row per common cytosine")
    ap.add_argument("-d", "--ref", dest="reffile", required=True, help="reference FASTA the reads were mapped to")
    ap.add_argument("--a", dest="a_files", nargs="+", required=True, metavar="FILE", help="mapping files of sample a, pooled")
    ap.add_argument("--b", dest="b_files", nargs="+", required=True, metavar="FILE", help="mapping files of sample b, pooled")
    ap.add_argument("--min-delta", dest="min_delta", type=fraction, default=0.0, metavar="X", help="least |ratio_b - ratio_a| of a listed cytosine, 0 .. 1 (default 0)")
    ap.add_argument("--max-p", dest="max_p", type=fraction, default=None, metavar="P", help="list only cytosines with a p-value of P or less (default: all)")
    ap.add_argument("--regions", dest="regions", default=None, metavar="BED", help="intervals (BED: name, start, end, optional label) to compare the pooled counts of")
    ap.add_argument("--region-out", dest="region_out", default=None, metavar="FILE", help="table to write for --regions, in the BED file's order")
    ap.add_argument("--bin", dest="bin", type=at_least(1, "a bin's width"), default=None, metavar="N", help="compare the pooled counts of every bin of N nt")
    ap.add_argument("--bin-out", dest="bin_out", default=None, metavar="FILE", help="table to write for --bin: the bins with a common cytosine")
    ap.add_argument("--fdr", dest="fdr", action="store_true", help="add the Benjamini-Hochberg q-value of every row to -o and --region-out")
    ap.add_argument("--max-q", dest="max_q", type=fraction, default=None, metavar="Q", help="list only cytosines with a q-value of Q or less; implies --fdr (default: all)")
    ap.add_argument("--dmr-out", dest="dmr_out", default=None, metavar="FILE", help="table of de novo differentially methylated regions to write")
    ap.add_argument("--dmr-max-q", dest="dmr_max_q", type=fraction, default=None, metavar="Q", help="a region's cytosines have a q-value of Q or less (default 0.05)")
    ap.add_argument("--dmr-max-gap", dest="dmr_max_gap", type=at_least(0, "the gap"), default=None, metavar="N",
                    help="a region's cytosines lie at most N nt behind one another (default 300)")
    ap.add_argument("--dmr-min-sites", dest="dmr_min_sites", type=at_least(1, "the number of cytosines"), default=None, metavar="K",
                    help="a region has at least K such cytosines (default 3)")
    ap.add_argument("-c", "--chr", dest="chroms", default="", help="comma-separated sequence names to keep (default: every sequence)")
    ap.add_argument("-u", "--unique", action="store_true", help="use uniquely mapped reads / pairs only")
    ap.add_argument("-p", "--pair", action="store_true", help="use properly paired mappings only")
    ap.add_argument("-q", "--quiet", action="store_true", help="no progress lines on stderr")
    ap.add_argument("-r", "--remove-duplicate", dest="rm_dup", action="store_true", help="keep the first read per fragment end and direction")
    ap.add_argument("-t", "--trim-fillin", dest="trim_fillin", type=int, default=2, help="end-repair nucleotides to ignore at fragment ends (default 2)")
    ap.add_argument("-g", "--combine-CpG", dest="combine_CpG", action="store_true", help="add the counts of the G of each CpG to its C")
    ap.add_argument("-m", "--min-depth", dest="min_depth", type=at_least(0, "the depth"), default=1, help="lowest depth a cytosine must have in both samples (default 1)")
    ap.add_argument("-x", "--context", dest="context", type=contexts, default=None, metavar="CG,CHG,CHH", help="compare cytosines of these contexts only (default: all)")
    ap.add_argument("-G", "--gpu", dest="device", type=int, default=0, help="GPU ordinal")
    ap.add_argument("--trim-5p", dest="trim5", type=at_least(0, "a number of cycles"), default=0, metavar="N", help="ignore the calls of the first N sequencing cycles of every read")
    ap.add_argument("--trim-3p", dest="trim3", type=at_least(0, "a number of cycles"), default=0, metavar="N", help="ignore the calls of the last N sequencing cycles of every read")
    ap.add_argument("--nonconv-filter", dest="nonconv_filter", type=at_least(0, "the threshold"), default=0, metavar="N",
                    help="drop reads with N or more methylated non-CpG calls (default 0: off)")
    return ap


def main(argv=None):
    """the command line: parses argv (default sys.argv[1:]) and prints run()'s summary line"""
    o = build_parser().parse_args(argv)
    sys.stdout.write(run(o.reffile, o.a_files, o.b_files, o.outfile, chroms=o.chroms.split(",") if o.chroms else None, unique=o.unique, pair=o.pair, rm_dup=o.rm_dup,
                         trim_fillin=o.trim_fillin, combine_CpG=o.combine_CpG, min_depth=o.min_depth, device=o.device, quiet=o.quiet, trim5=o.trim5, trim3=o.trim3,
                         context=o.context, nonconv_filter=o.nonconv_filter, min_delta=o.min_delta, max_p=o.max_p, regions=o.regions, region_out=o.region_out,
                         bin=o.bin, bin_out=o.bin_out, fdr=o.fdr, max_q=o.max_q, dmr_out=o.dmr_out, dmr_max_q=o.dmr_max_q, dmr_max_gap=o.dmr_max_gap,
                         dmr_min_sites=o.dmr_min_sites))


if __name__ == "__main__":
    main()
