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
import os
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

_VP, _U32, _I32, _U64, _STR = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64, C.c_char_p
# every bsx_meth_* prototype of include/bsx.h as name -> (restype, argtypes); tests/test_methratio_bind_cpu.py holds it against the header
PROTOTYPES = {
    "bsx_meth_create": (_I32, [_U32, _VP, _I32, _I32, C.POINTER(_VP)]),
    "bsx_meth_create_from_fasta": (_I32, [_STR, _STR, _I32, _I32, C.POINTER(_VP)]),
    "bsx_meth_n_chr": (_U32, [_VP]),
    "bsx_meth_chr_name": (_STR, [_VP, _U32]),
    "bsx_meth_destroy": (None, [_VP]),
    "bsx_meth_set_reference": (_I32, [_VP, _U32, _VP]),
    "bsx_meth_add": (_I32, [_VP, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32]),
    "bsx_meth_add_file": (_I32, [_VP, _STR, _I32, _VP, _I32, _I32, _U32, _VP]),
    "bsx_meth_set_cycle_trim": (_I32, [_VP, _U32, _U32]),
    "bsx_meth_set_mbias": (_I32, [_VP, _I32]),
    "bsx_meth_mbias_fetch": (_I32, [_VP, _VP, _VP]),
    "bsx_meth_write_mbias": (_I32, [_VP, _STR]),
    "bsx_meth_set_ct_snp": (_I32, [_VP, _I32]),
    "bsx_meth_set_contexts": (_I32, [_VP, _U32]),
    "bsx_meth_combine_cpg": (_I32, [_VP]),
    "bsx_meth_valid_mappings": (_I32, [_VP, _VP]),
    "bsx_meth_report_chr": (_I32, [_VP, _U32, _U32, _I32, _VP, _VP, _VP]),
    "bsx_meth_fetch_rows": (_I32, [_VP, _VP, _VP, _VP]),
    "bsx_meth_fetch_rows_snp": (_I32, [_VP, _VP, _VP]),
    "bsx_meth_write_table": (_I32, [_VP, _STR, _U32, _VP, _VP, _U32, _I32, _VP, _VP]),
    "bsx_meth_region_tile": (_U32, []),
    "bsx_meth_regions": (_I32, [_VP, _U32, _VP, _VP, _VP, _U32, _VP]),
    "bsx_meth_bins": (_I32, [_VP, _U32, _U32, _U32, _U64, _VP, _VP]),
    "bsx_meth_write_regions": (_I32, [_VP, _STR, _STR, _U32, _VP, _VP]),
    "bsx_meth_write_wig": (_I32, [_VP, _STR, _U32, _U32]),
    "bsx_meth_set_nonconv": (_I32, [_VP, _U32]),
    "bsx_meth_nonconv_dropped": (_I32, [_VP, _VP]),
    "bsx_meth_set_read_stats": (_I32, [_VP, _I32]),
    "bsx_meth_read_stats_fetch": (_I32, [_VP, _VP, _VP, _VP]),
    "bsx_meth_write_read_stats": (_I32, [_VP, _STR]),
    "bsx_meth_set_pdr": (_I32, [_VP, _U32]),
    "bsx_meth_pdr_report_chr": (_I32, [_VP, _U32, _U32, _VP]),
    "bsx_meth_pdr_fetch_rows": (_I32, [_VP, _VP, _VP, _VP]),
    "bsx_meth_write_pdr": (_I32, [_VP, _STR, _U32, _VP]),
    "bsx_meth_set_epi": (_I32, [_VP, _I32]),
    "bsx_meth_n_cpg": (_I32, [_VP, _U32, _VP]),
    "bsx_meth_epi_report_chr": (_I32, [_VP, _U32, _U32, _VP]),
    "bsx_meth_epi_fetch_rows": (_I32, [_VP, _VP, _VP]),
    "bsx_meth_write_epi": (_I32, [_VP, _STR, _U32, _VP]),
    "bsx_meth_diff_report_chr": (_I32, [_VP, _VP, _U32, _U32, _U32, _VP]),
    "bsx_meth_diff_fetch_rows": (_I32, [_VP, _VP, _VP, _VP]),
    "bsx_meth_write_diff": (_I32, [_VP, _VP, _STR, _U32, _U32, _VP, _VP]),
    "bsx_meth_diff_regions": (_I32, [_VP, _VP, _U32, _VP, _VP, _VP, _U32, _VP, _VP]),
    "bsx_meth_write_diff_regions": (_I32, [_VP, _VP, _STR, _STR, _U32, _VP, _VP]),
    "bsx_meth_write_diff_bins": (_I32, [_VP, _VP, _STR, _U32, _U32, _VP]),
    "bsx_meth_bh": (_I32, [_I32, _VP, _U64, _VP]),
    "bsx_meth_diff_report_all": (_I32, [_VP, _VP, _U32, _VP]),
    "bsx_meth_diff_fetch_all": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "bsx_meth_diff_dmrs": (_I32, [_VP, _VP, _U32, _VP, _U32, _U32, _U32, _VP]),
    "bsx_meth_diff_fetch_dmrs": (_I32, [_VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "bsx_meth_write_diff_fdr": (_I32, [_VP, _VP, _STR, _U32, _U32, _VP, _VP, _VP]),
    "bsx_meth_write_diff_regions_fdr": (_I32, [_VP, _VP, _STR, _STR, _U32, _VP, _VP]),
    "bsx_meth_write_dmrs": (_I32, [_VP, _VP, _STR, _U32, _VP, _U32, _U32, _U32, _VP]),
}
_path = os.fsencode  # str or os.PathLike -> the bytes of a const char *path


def _bind():
    """the library with PROTOTYPES applied (once)"""
    L = lib()
    if not getattr(L, "_meth_bound", False):
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
        L._meth_bound = True
    return L


def mbias_fetch(L, h):
    """the M-bias cells of a handle as uint64 [strand][context][cycle][unmethylated, methylated] and the count of calls beyond the last cycle"""
    cells, over = np.zeros((4, 4, MBIAS_CYCLES, 2), np.uint64), np.zeros(1, np.uint64)
    _check(L.bsx_meth_mbias_fetch(h, cells.ctypes.data, over.ctypes.data))
    return cells, int(over[0])


def read_stats_fetch(L, h):
    """the read histogram of a handle: cg[n_cg][m_cg] and ch[min(m_ch, 63)] as uint64, and the totals (reads, cg_over, ch_calls, ch_meth)"""
    cg, ch, tot = np.zeros((RS_CG, RS_CG), np.uint64), np.zeros(RS_CH, np.uint64), np.zeros(4, np.uint64)
    _check(L.bsx_meth_read_stats_fetch(h, cg.ctypes.data, ch.ctypes.data, tot.ctypes.data))
    return cg, ch, tuple(int(x) for x in tot)


def epi_fetch(L, h, chr, min_reads=1):
    """the epiallele rows of one sequence with at least min_reads reads: pos0 as uint32 [rows][4] (the 0-based positions of the four Cs) and counts as
    uint32 [rows][16] (by pattern: bit j set = CpG j of the window methylated)"""
    nr = np.zeros(1, np.uint32)
    _check(L.bsx_meth_epi_report_chr(h, chr, min_reads, nr.ctypes.data))
    pos0, counts = np.zeros((nr[0], 4), np.uint32), np.zeros((nr[0], 16), np.uint32)
    _check(L.bsx_meth_epi_fetch_rows(h, pos0.ctypes.data, counts.ctypes.data))
    return pos0, counts


def bh(p, device=0):
    """Benjamini-Hochberg q-values of the p-values `p` (float64, within 0 .. 1; a NaN is outside the family and stays NaN), computed on the device
    (bsx_meth_bh)"""
    p = np.ascontiguousarray(p, np.float64)
    if p.ndim != 1:
        raise ValueError("p must be one-dimensional")
    q = np.zeros(p.size, np.float64)
    _check(_bind().bsx_meth_bh(device, p.ctypes.data, p.size, q.ctypes.data))
    return q


class Meth:
    """one bsx_meth handle of include/bsx.h: the pile-up counters of a reference in HBM and every call on them (the methylation side's RefSeq / Batch).
    Methods check the return code and give numpy arrays.  `L` (the bound library) and `h` (the handle) are public: a test of the ABI's own error codes
    calls L.bsx_meth_*(h, ..) directly.  close() destroys the handle and sets h to None; it may be called again, and every other method of a closed object
    raises ValueError before any call into the library.  There is no __del__ (destruction sets the device and must not run at interpreter shutdown): use
    `with` or try / finally."""
    L = None
    h = None

    @classmethod
    def from_fasta(cls, path, chroms=None, rm_dup=False, device=0):
        """the sequences of a FASTA file (chroms: names to keep, default all) with their letters and names; rm_dup: with the fragment-end table of -r"""
        m = cls()
        m.L, h = _bind(), C.c_void_p()
        _check(m.L.bsx_meth_create_from_fasta(_path(path), ",".join(chroms).encode() if chroms else None, 1 if rm_dup else 0, device, C.byref(h)))
        m.h = h
        return m

    @classmethod
    def from_lengths(cls, lens, rm_dup=False, device=0):
        """sequences of the given lengths without names; set_reference gives each its letters"""
        m = cls()
        m.L, h, lens = _bind(), C.c_void_p(), np.array(lens, np.uint64)
        _check(m.L.bsx_meth_create(len(lens), lens.ctypes.data, 1 if rm_dup else 0, device, C.byref(h)))
        m.h = h
        return m

    def _live(self):
        if self.h is None:
            raise ValueError("this Meth is closed")
        return self.h

    def _call(self, name, *args):
        """L.<name>(h, *args) with the return code checked; a closed object raises before L is touched"""
        h = self._live()
        return _check(getattr(self.L, name)(h, *args))

    def _count(self, name, *args):
        """the same for a call whose last argument is a uint64 to fill, which is returned"""
        n = C.c_uint64()
        self._call(name, *args, C.byref(n))
        return n.value

    def close(self):
        if self.h is not None:
            self.L.bsx_meth_destroy(self.h)
            self.h = None

    def __enter__(self):
        self._live()
        return self

    def __exit__(self, *exc):
        self.close()

    def set_reference(self, chr, seq):
        """the upper-case letters of one sequence, as many as its length: str, bytes or a uint8 array (passed as it is, without a copy)"""
        h = self._live()
        seq = seq.encode() if isinstance(seq, str) else seq if isinstance(seq, bytes) else np.ascontiguousarray(seq, np.uint8)
        _check(self.L.bsx_meth_set_reference(h, chr, seq if isinstance(seq, bytes) else seq.ctypes.data))

    @property
    def n_chr(self):
        h = self._live()
        return self.L.bsx_meth_n_chr(h)

    def chr_name(self, c):
        """the name a FASTA gave sequence c ("" without one)"""
        h = self._live()
        return self.L.bsx_meth_chr_name(h, c).decode()

    # ---- settings (include/bsx.h says when each may change) ----
    def set_mbias(self, on=True): self._call("bsx_meth_set_mbias", 1 if on else 0)
    def set_cycle_trim(self, trim5, trim3): self._call("bsx_meth_set_cycle_trim", trim5, trim3)
    def set_contexts(self, mask): self._call("bsx_meth_set_contexts", mask)
    def set_nonconv(self, n): self._call("bsx_meth_set_nonconv", n)
    def set_read_stats(self, on=True): self._call("bsx_meth_set_read_stats", 1 if on else 0)
    def set_pdr(self, min_cpg): self._call("bsx_meth_set_pdr", min_cpg)
    def set_epi(self, on=True): self._call("bsx_meth_set_epi", 1 if on else 0)

    def set_ct_snp(self, mode):
        """mode: 0, 1, 2 or its name in CT_SNP_MODES"""
        self._call("bsx_meth_set_ct_snp", CT_SNP_MODES.index(mode) if isinstance(mode, str) else mode)

    # ---- input ----
    def add(self, alns, trim_fillin):
        """alns: [(chr id, 0-based pos, strand code, insert, cut_at or -1, letters)] in input order; an empty list is no call"""
        self._live()
        if not alns:
            return
        off = np.cumsum([0] + [len(a[5]) for a in alns]).astype(np.uint64)
        seq = np.frombuffer("".join(a[5] for a in alns).encode() + b"\0", np.uint8)
        col = lambda k, dtype: np.array([a[k] for a in alns], dtype)
        self.add_arrays(len(alns), col(0, np.uint32), col(1, np.int64), col(2, np.uint8), col(3, np.int32), col(4, np.int64), seq, off, trim_fillin)

    def add_arrays(self, n, chr, pos, strand, insert, cut_at, seq, off, trim_fillin):
        """the first n alignments of the arrays of bsx_meth_add (uint32, int64, uint8, int32, int64; letters as uint8 with uint64 offsets[n + 1]).  An array of
        that type goes to the library as it is; another one is converted"""
        self._live()
        a = [np.ascontiguousarray(x, t) for x, t in zip((chr, pos, strand, insert, cut_at, seq, off), (np.uint32, np.int64, np.uint8, np.int32, np.int64, np.uint8, np.uint64))]
        self._call("bsx_meth_add", n, *[x.ctypes.data for x in a], trim_fillin)

    def add_file(self, path, unique=False, pair=False, trim_fillin=2):
        """a mapping file of bsmap, *.sam / *.bam by their format and anything else as BSP; returns its lines"""
        self._live()
        ext = str(path)[-4:].upper()
        return self._count("bsx_meth_add_file", _path(path), 2 if ext == ".BAM" else 1 if ext == ".SAM" else 0, None, 1 if unique else 0, 1 if pair else 0, trim_fillin)

    # ---- counters ----
    def combine_cpg(self): self._call("bsx_meth_combine_cpg")
    def valid_mappings(self): return self._count("bsx_meth_valid_mappings")
    def nonconv_dropped(self): return self._count("bsx_meth_nonconv_dropped")
    def n_cpg(self, c): return self._count("bsx_meth_n_cpg", c)

    # ---- reports: one sequence's rows as uint32 arrays ----
    def report(self, c, min_depth=1, meth0=True, snp=False):
        """(pos0, depth, meth, n_covered, sum_depth) of sequence c, with snp=True (pos0, depth, meth, rev_g, rev_ga, n_covered, sum_depth)"""
        h, nr, cov, sd = self._live(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(self.L.bsx_meth_report_chr(h, c, min_depth, 1 if meth0 else 0, C.byref(nr), C.byref(cov), C.byref(sd)))
        rows = [np.zeros(nr.value, np.uint32) for _ in range(5 if snp else 3)]
        _check(self.L.bsx_meth_fetch_rows(h, *[x.ctypes.data for x in rows[:3]]))
        if snp:
            _check(self.L.bsx_meth_fetch_rows_snp(h, rows[3].ctypes.data, rows[4].ctypes.data))
        return (*rows, cov.value, sd.value)

    def pdr_report(self, c, min_reads=1):
        """(pos0, reads, discordant) of sequence c"""
        h, nr = self._live(), C.c_uint32()
        _check(self.L.bsx_meth_pdr_report_chr(h, c, min_reads, C.byref(nr)))
        rows = [np.zeros(nr.value, np.uint32) for _ in range(3)]
        _check(self.L.bsx_meth_pdr_fetch_rows(h, *[x.ctypes.data for x in rows]))
        return tuple(rows)

    def epi_report(self, c, min_reads=1): return epi_fetch(self.L, self._live(), c, min_reads)   # (pos0 [rows][4], counts [rows][16]) of sequence c
    def mbias(self): return mbias_fetch(self.L, self._live())
    def read_stats(self): return read_stats_fetch(self.L, self._live())

    def bins(self, c, width, min_depth=1):
        """the sums N, M, D, E, MC of every bin of `width` positions of sequence c as uint64 [bins][5]"""
        h, n = self._live(), C.c_uint64()
        self.L.bsx_meth_bins(h, c, width, min_depth, 0, None, C.byref(n))   # the size query: an error code by design, with n set
        out = np.zeros((n.value, 5), np.uint64)
        _check(self.L.bsx_meth_bins(h, c, width, min_depth, n.value, out.ctypes.data, C.byref(n)))
        return out[:n.value]

    def regions(self, chr, start, end, min_depth=1):
        """the same sums over the intervals [start[i], end[i]) of sequence chr[i], as uint64 [len(chr)][5]"""
        h = self._live()
        a = [np.ascontiguousarray(x, np.uint32) for x in (chr, start, end)]
        if not a[0].size == a[1].size == a[2].size:
            raise ValueError("chr, start and end differ in length")
        out = np.zeros((a[0].size, 5), np.uint64)
        _check(self.L.bsx_meth_regions(h, a[0].size, *[x.ctypes.data for x in a], min_depth, out.ctypes.data))
        return out

    # ---- files ----
    def write_table(self, path, min_depth=1, meth0=True):
        """the table of every sequence in sorted name order; returns (n_covered, sum_depth) of the summary line"""
        h, nc, nd = self._live(), C.c_uint64(), C.c_uint64()
        _check(self.L.bsx_meth_write_table(h, _path(path), 0, None, None, min_depth, 1 if meth0 else 0, C.byref(nc), C.byref(nd)))
        return nc.value, nd.value

    def write_mbias(self, path): self._call("bsx_meth_write_mbias", _path(path))
    def write_read_stats(self, path): self._call("bsx_meth_write_read_stats", _path(path))
    def write_wig(self, path, width, min_depth=1): self._call("bsx_meth_write_wig", _path(path), width, min_depth)
    def write_pdr(self, path, min_reads=1): return self._count("bsx_meth_write_pdr", _path(path), min_reads)   # the rows written
    def write_epi(self, path, min_reads=1): return self._count("bsx_meth_write_epi", _path(path), min_reads)   # the rows written

    def write_regions(self, bed_path, out_path, min_depth=1):
        """one pooled ratio per interval of a BED file; returns (intervals written, intervals dropped: on sequences that are not loaded)"""
        h, nw, nd = self._live(), C.c_uint64(), C.c_uint64()
        _check(self.L.bsx_meth_write_regions(h, _path(bed_path), _path(out_path), min_depth, C.byref(nw), C.byref(nd)))
        return nw.value, nd.value

    # ---- two samples: self is sample A, other sample B; no call changes a counter of either ----
    def _pair(self, other):
        """(A's handle, B's handle): self is checked first, then other"""
        h = self._live()
        return h, other._live()

    def diff_report(self, other, c, min_depth=1, min_delta_permille=0):
        """the common sites of sequence c whose ratios differ by min_delta_permille / 1000 or more: (pos0 uint32, counts uint32 [rows][4] = mA, dA, mB, dB,
        p float64: the two-sided Fisher exact test of every row)"""
        (h, hb), nr = self._pair(other), C.c_uint32()
        _check(self.L.bsx_meth_diff_report_chr(h, hb, c, min_depth, min_delta_permille, C.byref(nr)))
        pos0, counts, p = np.zeros(nr.value, np.uint32), np.zeros((nr.value, 4), np.uint32), np.zeros(nr.value, np.float64)
        _check(self.L.bsx_meth_diff_fetch_rows(h, pos0.ctypes.data, counts.ctypes.data, p.ctypes.data))
        return pos0, counts, p

    def diff_regions(self, other, chr, start, end, min_depth=1):
        """(sums uint64 [len(chr)][5] = N, MA, DA, MB, DB over the common sites of every interval, p float64: the test on the sums, NaN where N is 0)"""
        h, hb = self._pair(other)
        a = [np.ascontiguousarray(x, np.uint32) for x in (chr, start, end)]
        if not a[0].size == a[1].size == a[2].size:
            raise ValueError("chr, start and end differ in length")
        sums, p = np.zeros((a[0].size, 5), np.uint64), np.zeros(a[0].size, np.float64)
        _check(self.L.bsx_meth_diff_regions(h, hb, a[0].size, *[x.ctypes.data for x in a], min_depth, sums.ctypes.data, p.ctypes.data))
        return sums, p

    def write_diff(self, other, path, min_depth=1, min_delta_permille=0, max_p=None, max_q=None, fdr=False):
        """the rows of every sequence in sorted name order, with max_p those with p <= max_p; returns the rows written.  fdr (or a max_q): with the
        Benjamini-Hochberg q of every row over all common sites as a 13th column, and with max_q only the rows with q <= max_q"""
        (h, hb), n = self._pair(other), C.c_uint64()
        ref = lambda x: None if x is None else C.byref(C.c_double(x))
        if fdr or max_q is not None:
            _check(self.L.bsx_meth_write_diff_fdr(h, hb, _path(path), min_depth, min_delta_permille, ref(max_p), ref(max_q), C.byref(n)))
        else:
            _check(self.L.bsx_meth_write_diff(h, hb, _path(path), min_depth, min_delta_permille, ref(max_p), C.byref(n)))
        return n.value

    def write_diff_regions(self, other, bed_path, out_path, min_depth=1, fdr=False):
        """one row per interval of a BED file; returns (intervals written, intervals dropped: on sequences that are not loaded).  fdr: with the q of every
        interval over the file's intervals that hold a common site"""
        (h, hb), nw, nd = self._pair(other), C.c_uint64(), C.c_uint64()
        write = self.L.bsx_meth_write_diff_regions_fdr if fdr else self.L.bsx_meth_write_diff_regions
        _check(write(h, hb, _path(bed_path), _path(out_path), min_depth, C.byref(nw), C.byref(nd)))
        return nw.value, nd.value

    # ---- q-values over all rows and de novo DMRs ----
    def write_order(self):
        """the sequence ids in the order the diff files and the store list them: sorted names, the ids' own order without names"""
        n = self.n_chr
        names = [self.chr_name(c) for c in range(n)]
        return sorted(range(n), key=lambda c: names[c].encode()) if all(names) else list(range(n))

    def diff_report_all(self, other, min_depth=1):
        """every common site of every sequence, in write_order() and ascending position: (row_start uint32 [n_chr + 1] by rank in that order, pos0 uint32,
        counts uint32 [rows][4] = mA, dA, mB, dB, cls uint8, p float64, q float64: Benjamini-Hochberg over all rows).  The rows stay on the device as
        the store diff_dmrs works on"""
        (h, hb), n = self._pair(other), C.c_uint64()
        _check(self.L.bsx_meth_diff_report_all(h, hb, min_depth, C.byref(n)))
        rows = n.value
        row_start, pos0, counts, cls = np.zeros(self.n_chr + 1, np.uint32), np.zeros(rows, np.uint32), np.zeros((rows, 4), np.uint32), np.zeros(rows, np.uint8)
        p, q = np.zeros(rows, np.float64), np.zeros(rows, np.float64)
        _check(self.L.bsx_meth_diff_fetch_all(h, *[x.ctypes.data for x in (row_start, pos0, counts, cls, p, q)]))
        return row_start, pos0, counts, cls, p, q

    def diff_dmrs(self, other, max_q, min_delta_permille=0, max_gap=300, min_sites=3, min_depth=1):
        """the DMRs over the store of the last diff_report_all(other, min_depth): (chr uint32, start uint32, end uint32, n_sig uint32, sums uint64 [n][5] =
        N, MA, DA, MB, DB over all common sites of [start, end), p float64: the test on the sums)"""
        (h, hb), n = self._pair(other), C.c_uint32()
        _check(self.L.bsx_meth_diff_dmrs(h, hb, min_depth, C.byref(C.c_double(max_q)), min_delta_permille, max_gap, min_sites, C.byref(n)))
        cols = [np.zeros(n.value, np.uint32) for _ in range(4)] + [np.zeros((n.value, 5), np.uint64), np.zeros(n.value, np.float64)]
        _check(self.L.bsx_meth_diff_fetch_dmrs(h, *[x.ctypes.data for x in cols]))
        return tuple(cols)

    def write_dmrs(self, other, path, max_q=0.05, min_delta_permille=0, max_gap=300, min_sites=3, min_depth=1):
        """the DMRs as a file (the store is built unless one stands for other and min_depth); returns the DMRs written"""
        (h, hb), n = self._pair(other), C.c_uint64()
        _check(self.L.bsx_meth_write_dmrs(h, hb, _path(path), min_depth, C.byref(C.c_double(max_q)), min_delta_permille, max_gap, min_sites, C.byref(n)))
        return n.value

    def write_diff_bins(self, other, path, width, min_depth=1):
        """one row per bin of `width` positions that holds a common site; returns the rows written"""
        (h, hb), n = self._pair(other), C.c_uint64()
        _check(self.L.bsx_meth_write_diff_bins(h, hb, _path(path), width, min_depth, C.byref(n)))
        return n.value


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

    disp("reading reference %s ..." % reffile)
    with Meth.from_fasta(reffile, chroms, rm_dup, device) as m:
        if mbias:
            m.set_mbias()
        if trim5 or trim3:
            m.set_cycle_trim(trim5, trim3)
        if ct_snp != "no-action":
            m.set_ct_snp(ct_snp)
        if context is not None:
            m.set_contexts(sum(CONTEXT_BITS[x] for x in set(context)))
        if nonconv_filter:
            m.set_nonconv(nonconv_filter)
        if read_stats is not None:
            m.set_read_stats()
        if pdr is not None:
            m.set_pdr(pdr_min_cpg)
        if epi is not None:
            m.set_epi()
        for infile in infiles:
            disp("reading %s ..." % infile)
            m.add_file(infile, unique, pair, max(0, trim_fillin))
        if mbias:
            disp("writing %s ..." % mbias)
            m.write_mbias(mbias)
        if nonconv_filter:
            disp("%d reads with %d or more methylated non-CpG calls dropped" % (m.nonconv_dropped(), nonconv_filter))
        if read_stats is not None:
            disp("writing %s ..." % read_stats)
            m.write_read_stats(read_stats)
        if combine_CpG:
            disp("combining CpG methylation from both strands ...")
            m.combine_cpg()
        disp("writing %s ..." % outfile)
        nc, nd = m.write_table(outfile, min_depth, meth0)
        nmap = m.valid_mappings()
        if pdr is not None:
            disp("writing %s ..." % pdr)
            m.write_pdr(pdr, pdr_min_reads)
        if epi is not None:
            disp("writing %s ..." % epi)
            m.write_epi(epi, epi_min_reads)
        if wig is not None:
            disp("writing %s ..." % wig)
            m.write_wig(wig, wig_bin, min_depth)
        if regions is not None:
            disp("writing %s ..." % region_out)
            nw, ndrop = m.write_regions(regions, region_out, min_depth)
            disp("%d intervals of %s written, %d on sequences that are not loaded dropped" % (nw, regions, ndrop))
        disp("done.")
        # (with nothing covered the reference dies here on a division by zero; that is reported instead)
        if nc == 0:
            return "total %d valid mappings, 0 covered cytosines.\n" % nmap
        return "total %d valid mappings, %d covered cytosines, average coverage: %.2f fold.\n" % (nmap, nc, float(nd) / nc)


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
