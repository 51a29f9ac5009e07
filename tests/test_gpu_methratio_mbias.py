"""M-bias tally and cycle trimming of bsmap_amd.methratio (bsx_meth_set_mbias / _set_cycle_trim / _mbias_fetch / _write_mbias,
--mbias / --trim-5p / --trim-3p) against a pure-Python model written here.

The model restates the reference script's per-alignment code (its methratio.py:31-65 and :100-113) on parsed tuples, with Python's
own slices, and adds the three rules of this feature:
  cycle    the letter's 0-based index in the untrimmed read in sequencing direction: j for '++' / '--', n0-1-j for '-+' / '+-'
  context  from the upper-case reference inside the chromosome: next two letters on '+' strands, previous two (C in the role of G)
           on '-' strands; 0 CG, 1 CHG, 2 CHH, 3 everything else (a letter outside ACGT or a neighbour beyond the chromosome)
  mask     a call at cycle c of a read of n0 letters is dropped when c < trim5 or c >= n0 - trim3; nothing else changes
It never looks at the library's output."""
import ctypes as C
import gzip
import json
import os
import re

import numpy as np
import pytest

import golden_util as G
import meth_util as U

pytestmark = pytest.mark.gpu
STRANDS = ("++", "-+", "+-", "--")  # the library's strand codes 0..3
CONTEXTS = ("CG", "CHG", "CHH", "CN")
CYCLES = 1024
BSX_ERR_STATE = -5


# ---- the model ------------------------------------------------------------------------------------------------------
def context_class(refseq, g, plus):
    """class of the cytosine at refseq[g] ('C' on the '+' strand, 'G' on the '-' strand)"""
    if plus:
        n1 = refseq[g + 1] if g + 1 < len(refseq) else ""
        n2 = refseq[g + 2] if g + 2 < len(refseq) else ""
        gl, h = "G", "ACT"
    else:
        n1 = refseq[g - 1] if g - 1 >= 0 else ""
        n2 = refseq[g - 2] if g - 2 >= 0 else ""
        gl, h = "C", "AGT"
    if n1 == gl:
        return 0
    if n1 and n1 in h:
        if n2 == gl:
            return 1
        if n2 and n2 in h:
            return 2
    return 3


def model(refs, alns, trim_fillin=2, rm_dup=False, trim5=0, trim3=0):
    """refs: upper-case chromosome strings in id order; alns: (chr id, 0-based pos, strand code, insert, cut_at or -1, letters) in
    input order.  Returns depth, meth (per chromosome lists), cells [4][4][CYCLES][2], calls beyond CYCLES, valid mappings."""
    depth = [[0] * len(r) for r in refs]
    meth = [[0] * len(r) for r in refs]
    coverage = [[0] * len(r) for r in refs]
    cells = np.zeros((4, 4, CYCLES, 2), np.uint64)
    over = nmap = 0
    for c, pos, st, insert, cut_at, letters in alns:
        strand, n0 = STRANDS[st], len(letters)
        seq = list(enumerate(letters))  # (index in the untrimmed read, letter): sliced like the script slices its string
        if rm_dup:  # methratio.py:52-56
            if strand == "+-" or strand == "-+":
                frag_end, direction = pos + len(seq), 2
            else:
                frag_end, direction = pos, 1
            if 0 <= frag_end < len(refs[c]):  # (outside, the script dies on its coverage array; the library applies no filter there)
                if coverage[c][frag_end] & direction:
                    continue
                coverage[c][frag_end] |= direction
        if trim_fillin > 0:  # methratio.py:57-63
            if strand == "+-":
                seq = seq[:-trim_fillin]
            elif strand == "--":
                seq, pos = seq[trim_fillin:], pos + trim_fillin
            elif insert != 0 and len(seq) > abs(insert) - trim_fillin:
                trim_nt = len(seq) - (abs(insert) - trim_fillin)
                if strand == "++":
                    seq = seq[:-trim_nt]
                elif strand == "-+":
                    seq, pos = seq[trim_nt:], pos + trim_nt
        if cut_at >= 0:  # methratio.py:64, cut_at = PNEXT-1 of a SAM record with insert > 0
            seq = seq[:cut_at - pos]
        if pos + len(seq) > len(refs[c]):  # methratio.py:102
            continue
        nmap += 1
        assert pos >= 0
        match, convert = ("C", "T") if strand[0] == "+" else ("G", "A")
        for k, (j, ch) in enumerate(seq):  # methratio.py:105-113
            g = pos + k
            if refs[c][g] != match or ch not in (match, convert):
                continue
            cycle = j if strand in ("++", "--") else n0 - 1 - j
            if cycle < trim5 or cycle >= n0 - trim3:
                continue
            m = 1 if ch == match else 0
            depth[c][g] += 1
            meth[c][g] += m
            if cycle >= CYCLES:
                over += 1
            else:
                cells[st, context_class(refs[c], g, strand[0] == "+"), cycle, m] += 1
    return depth, meth, cells, over, nmap


def model_rows(depth, meth):
    return [(c, g, d, meth[c][g]) for c in range(len(depth)) for g, d in enumerate(depth[c]) if d >= 1]


# ---- the library through bsmap_amd.methratio.Meth ---------------------------------------------------------------------------
def handle(fa, rm_dup=False, mbias=True, trim=None):
    return U.open_meth(fa, rm_dup, mbias=mbias, trim=trim)


def got_rows(h, n_chr):
    return U.table_rows(h, n_chr)[0]


def got_table(h, path):
    return U.written_table(h, path)[0].encode()


# ---- the edge set of tests 1 and 5 ---------------------------------------------------------------------------------------
class Edges:
    """two chromosomes of 301 and 97 letters: each begins and ends with C or G, has an N beside a C, lower case in the FASTA; the
    second begins with G, so a C that ends the first must not pair with it.  About 400 alignments: four strands, lengths 1, 2, 63,
    64, 65, 128, 129, 144, at position 0, at clen - len, one letter further (invalid) and in between, inserts on both sides of the
    '++' / '-+' trim, cut_at inside, behind and in front of the read, and repeated fragments for -r."""
    LENGTHS = (1, 2, 63, 64, 65, 128, 129, 144)

    def __init__(self):
        rng = np.random.default_rng(20)
        self.names, self.refs = ["edgeA", "edgeB"], []
        for n, first, last in ((301, "C", "C"), (97, "G", "G")):
            s = rng.choice(list("ACGT"), n).tolist()
            s[0], s[-1] = first, last
            s[20:25] = list("ACNCG")    # an N behind a C ('+' context) ...
            s[40:45] = list("TGNGA")    # ... and in front of a G ('-' context)
            s[60:64] = list("CCGG")
            self.refs.append("".join(s))
        assert self.refs[0][-1] == "C" and self.refs[1][0] == "G"
        low = lambda s: s[:10] + s[10:50].lower() + s[50:]
        self.fasta = "".join(">%s some text\n%s" % (n, "".join(low(s)[i:i + 50] + "\n" for i in range(0, len(s), 50))) for n, s in zip(self.names, self.refs))
        assert self.fasta != self.fasta.upper()
        alns = []
        k = 0
        for rep in range(2):
            for c, ref in enumerate(self.refs):
                for L in self.LENGTHS:
                    if L > len(ref):
                        continue
                    for st in range(4):
                        for pos in (0, len(ref) - L) + tuple(rng.integers(0, len(ref) - L + 1, 2 - rep).tolist()):
                            k += 1
                            insert = (0, L + 1, L - 3, -(L - 3), 250, L + 7, -L)[k % 7]
                            cut = (-1, -1, pos + L // 2, pos + L + 5, -1, max(pos - 2, 0), -1, pos + L - 1, -1)[k % 9] if insert > 0 else -1
                            alns.append((c, pos, st, insert, cut, self.read(rng, c, pos, L, st)))
        for c, ref in enumerate(self.refs):  # 64 letters from clen - 63: one letter past the end unless a trim takes it off
            for st in (0, 3, 1, 2):
                alns.append((c, len(ref) - 63, st, 0, -1, self.read(rng, c, len(ref) - 64, 64, st)))
        for i in rng.integers(0, len(alns), 40).tolist():  # the same fragment with other letters: -r has to keep the first
            c, pos, st, insert, cut, s = alns[i]
            alns.append((c, pos, st, insert, cut, self.read(rng, c, pos, len(s), st)))
        order = rng.permutation(len(alns)).tolist()
        self.alns = [alns[i] for i in order]
        assert 380 <= len(self.alns) <= 440, len(self.alns)
        self._model = {}

    def read(self, rng, c, pos, L, st):
        ref = self.refs[c]
        x = [ref[min(pos + i, len(ref) - 1)] for i in range(L)]
        match, convert = ("C", "T") if st % 2 == 0 else ("G", "A")
        for i in range(L):
            r = rng.random()
            if x[i] == "N":
                x[i] = "ACGT"[int(rng.integers(0, 4))]
            if x[i] == match and r < 0.5:
                x[i] = convert
            elif r > 0.96:
                x[i] = "ACGTN"[int(rng.integers(0, 5))]
        return "".join(x)

    def model(self, trim_fillin, rm_dup, trim5=0, trim3=0):
        key = (trim_fillin, rm_dup, trim5, trim3)
        if key not in self._model:
            self._model[key] = model(self.refs, self.alns, trim_fillin, rm_dup, trim5, trim3)
        return self._model[key]


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    e = Edges()
    e.dir = tmp_path_factory.mktemp("mbias_edges")
    e.fa = str(e.dir / "edges.fa")
    open(e.fa, "w").write(e.fasta)
    return e


def test_edge_set_covers_what_it_claims(edges):
    """the generated set really holds the shapes the other tests rely on (checked on the model's side only)"""
    depth, meth, cells, over, nmap = edges.model(2, False)
    assert over == 0 and 0 < nmap < len(edges.alns)            # some alignments are invalid
    assert all(cells[s].sum() > 0 for s in range(4))
    assert all(cells[:, x].sum() > 0 for x in range(4))       # every context class, CN included
    assert cells[:, :, 143].sum() > 0 and cells[:, :, 144:].sum() == 0
    assert edges.model(2, True)[4] < nmap                      # -r removes something
    assert depth[0][300] > 0 and depth[1][0] > 0 and depth[1][96] > 0 and depth[0][0] > 0  # both ends of both chromosomes are called
    assert context_class(edges.refs[0], 300, True) == 3 and context_class(edges.refs[1], 0, False) == 3


# ---- 1. model parity on edge shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rm_dup", [0, 1])
@pytest.mark.parametrize("trim_fillin", [0, 2, 5])
def test_model_parity_on_edge_shapes(edges, trim_fillin, rm_dup):
    depth, meth, cells, over, nmap = edges.model(trim_fillin, bool(rm_dup))
    with handle(edges.fa, rm_dup) as h:
        h.add(edges.alns, trim_fillin)
        got_cells, got_over = h.mbias()
        assert got_over == over
        assert np.array_equal(got_cells, cells), np.argwhere(got_cells != cells)[:8].tolist()
        assert got_rows(h, 2) == model_rows(depth, meth)
        assert h.valid_mappings() == nmap


# ---- 2. sum invariant against the pinned table ------------------------------------------------------------------------------
GOLD = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio.json.gz"), "rt"))
ALL_RUNS = [(c, i) for c in sorted(GOLD["cases"]) for i in range(len(GOLD["cases"][c]["runs"]))]
RUNS = [(c, i) for c, i in ALL_RUNS if "-g" not in GOLD["cases"][c]["runs"][i]["options"]]


@pytest.fixture(scope="module")
def gold_files(tmp_path_factory):
    import base64
    d = tmp_path_factory.mktemp("mbias_gold")
    fa = str(d / "g.fa")
    open(fa, "w").write(GOLD["fasta"])
    paths = {}
    for c, case in GOLD["cases"].items():
        for fn, txt in case["files"].items():
            open(str(d / fn), "w").write(txt)
        for fn, b64 in case.get("files_b64", {}).items():
            open(str(d / fn), "wb").write(base64.b64decode(b64))
        paths[c] = [str(d / fn) for fn in case["infiles"]]
    return fa, paths, d


def parse_mbias(text):
    """the file of bsx_meth_write_mbias: cells [4][4][CYCLES][2], calls beyond the last cycle, Lmax, the data rows and the comment lines"""
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0] == "strand\tcontext\tcycle\tmeth\tdepth\tratio"
    rows = [l.split("\t") for l in lines[1:-1] if not l.startswith("#")]
    comments = [l for l in lines[1:-1] if l.startswith("#")]
    assert lines[1:-1] == ["\t".join(r) for r in rows] + comments  # the comment lines come last
    cells = np.zeros((4, 4, CYCLES, 2), np.uint64)
    for s, x, cyc, m, d, ratio in rows:
        m, d = int(m), int(d)
        cells[STRANDS.index(s), CONTEXTS.index(x), int(cyc) - 1] = (d - m, m)
        assert ratio == ("NA" if d == 0 else "%.3f" % (float(m) / d))
    over = int(re.fullmatch(r"# calls beyond cycle 1024: (\d+)", comments[-1]).group(1))
    return cells, over, len(rows) // 16, rows, comments


def test_g_cases_are_a_minority_of_the_fixture():
    n_g = len(ALL_RUNS) - len(RUNS)
    assert 0 < n_g * 2 < len(ALL_RUNS), f"{n_g} of {len(ALL_RUNS)} runs of tests/golden/methratio.json.gz have -g and are left out of the sum invariant"


@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{'_'.join(GOLD['cases'][c]['runs'][i]['options']) or 'default'}" for c, i in RUNS])
def test_sum_invariant_against_the_pinned_table(case, i, gold_files, capsys):
    from bsmap_amd import methratio
    fa, paths, d = gold_files
    run = GOLD["cases"][case]["runs"][i]
    opts = list(run["options"])
    if "same_as" in run:  # a BAM twin of that case's SAM file: same expected output
        run = [r for r in GOLD["cases"][run["same_as"]]["runs"] if r["options"] == run["options"]][0]
    out, mb = str(d / f"{case}_{i}.txt"), str(d / f"{case}_{i}.mbias")
    methratio.main(["-q", "-o", out, "-d", fa] + opts + ["--mbias", mb] + paths[case])
    assert open(out).read() == run["table"]            # M-bias on: the table is still the reference script's
    if not run["crashed"]:
        assert capsys.readouterr().out == run["stdout"]
    methratio.main(["-q", "-o", out, "-d", fa] + opts + ["-z", "-m", "1", "--mbias", mb] + paths[case])
    capsys.readouterr()
    rows = [l.split("\t") for l in open(out).read().split("\n")[1:] if l]
    cells, over, lmax, _, _ = parse_mbias(open(mb).read())
    assert over == 0
    assert int(cells.sum()) == sum(int(f[5]) for f in rows)              # every call of depth is in exactly one cell
    assert int(cells[..., 1].sum()) == sum(int(f[6]) for f in rows)      # ... and every methylated call in a methylated cell
    if rows:
        assert lmax > 0


# ---- 3. contention and flush ------------------------------------------------------------------------------------------------
def test_contention_and_flush(tmp_path):
    """2^16 copies of one '+-' alignment of 300 letters (cycles below and above the block-private extent), no -r, in one
    bsx_meth_add call and split over three: every cell is 65 536 x the model's single-alignment cell"""
    rng = np.random.default_rng(5)
    ref = "".join(rng.choice(list("ACGT"), 400).tolist())
    fa = str(tmp_path / "one.fa")
    open(fa, "w").write(">one\n" + ref + "\n")
    read = "".join(("T" if (ch == "C" and i % 3 == 0) else ch) for i, ch in enumerate(ref[50:350]))
    aln = (0, 50, 2, 0, -1, read)
    depth, meth, cells, over, nmap = model([ref], [aln], 2)
    assert nmap == 1 and cells[2, :, 256:].sum() > 0 and cells[2, :, :256].sum() > 0 and cells[2, :, :, 0].sum() > 0 and cells[2, :, :, 1].sum() > 0
    n = 1 << 16
    got = []
    for split in ((n,), (1, 30_000, n - 30_001)):
        with handle(fa) as h:
            for part in split:
                h.add([aln] * part, 2)
            got.append((h.mbias(), got_rows(h, 1), h.valid_mappings()))
    for (got_cells, got_over), rows, got_nmap in got:
        assert got_over == 0 and got_nmap == n
        assert np.array_equal(got_cells, cells * np.uint64(n))
        assert rows == [(c, g, d * n, m * n) for c, g, d, m in model_rows(depth, meth)]
    assert np.array_equal(got[0][0][0], got[1][0][0]) and got[0][1] == got[1][1]


# ---- 4. beyond the cap --------------------------------------------------------------------------------------------------------
def test_beyond_the_cap(tmp_path):
    """one SAM read of 1 030 letters on a chromosome of 1 100, strands '++' and '-+': cycles from 1 024 on go to the overflow count"""
    rng = np.random.default_rng(6)
    ref = "".join(rng.choice(list("ACGT"), 1100).tolist())
    fa, sam = str(tmp_path / "long.fa"), str(tmp_path / "long.sam")
    open(fa, "w").write(">long\n" + "".join(ref[i:i + 70] + "\n" for i in range(0, 1100, 70)))
    alns, lines = [], ["@SQ\tSN:long\tLN:1100\n"]
    for k, (st, pos) in enumerate(((0, 30), (1, 70))):
        match, convert = ("C", "T") if st == 0 else ("G", "A")
        read = "".join((convert if (ch == match and i % 2) else ch) for i, ch in enumerate(ref[pos:pos + 1030]))
        alns.append((0, pos, st, 0, -1, read))
        lines.append("r%d\t%d\tlong\t%d\t255\t1030M\t*\t0\t0\t%s\t%s\tNM:i:0\tZS:Z:%s\n" % (k, 0 if st == 0 else 16, pos + 1, read, "I" * 1030, STRANDS[st]))
    open(sam, "w").write("".join(lines))
    depth, meth, cells, over, nmap = model([ref], alns, 2)
    # both strands have calls beyond the cap, just below it, above the block-private extent and in the first cycles
    assert nmap == 2 and over >= 2 and all(cells[st, :, a:b].sum() > 0 for st in (0, 1) for a, b in ((0, 16), (256, 1024), (1008, 1024)))
    assert sum(1 for _, pos, st, _, _, read in alns for j in range(1030) if (j if st == 0 else 1029 - j) >= 1024
               and ref[pos + j] == "CG"[st] and read[j] in ("CT", "GA")[st]) == over
    with handle(fa) as h:
        h.add_file(sam)
        got_cells, got_over = h.mbias()
        assert got_over == over
        assert np.array_equal(got_cells, cells)
        assert got_rows(h, 1) == model_rows(depth, meth) and h.valid_mappings() == 2


# ---- 5. cycle trimming ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trim5,trim3", [(0, 0), (3, 0), (0, 4), (5, 5), (200, 0)])
def test_cycle_trimming(edges, trim5, trim3):
    for trim_fillin, rm_dup in ((2, 1), (0, 0)):
        depth, meth, cells, over, nmap = edges.model(trim_fillin, bool(rm_dup), trim5, trim3)
        with handle(edges.fa, rm_dup, trim=(trim5, trim3)) as h:
            h.add(edges.alns, trim_fillin)
            got_cells, got_over = h.mbias()
            assert got_over == over and np.array_equal(got_cells, cells)
            rows = got_rows(h, 2)
            assert rows == model_rows(depth, meth)
            assert h.valid_mappings() == nmap == edges.model(trim_fillin, bool(rm_dup))[4]  # masking calls never changes what counts as a valid mapping
            table = got_table(h, str(edges.dir / "trim.txt"))
        if (trim5, trim3) == (0, 0):
            with handle(edges.fa, rm_dup, mbias=False) as h:  # neither new call made
                h.add(edges.alns, trim_fillin)
                assert got_table(h, str(edges.dir / "plain.txt")) == table and h.valid_mappings() == nmap
            assert len(rows) > 100
        if (trim5, trim3) == (200, 0):
            assert rows == [] and nmap > 200 and table == b"chr\tpos\tstrand\tcontext\tratio\ttotal_C\tmethy_C\tCI_lower\tCI_upper\n"
        if (trim5, trim3) == (5, 5):
            assert got_cells[:, :, :5].sum() == 0 and got_cells.sum() > 0


# ---- 6. state rules ---------------------------------------------------------------------------------------------------------------
def test_state_rules(edges):
    cells = np.zeros((4, 4, CYCLES, 2), np.uint64)
    over = C.c_uint64()
    with handle(edges.fa, mbias=False) as h:
        fetch = lambda: h.L.bsx_meth_mbias_fetch(h.h, cells.ctypes.data, C.byref(over))
        assert fetch() == BSX_ERR_STATE                                   # M-bias off
        assert h.L.bsx_meth_write_mbias(h.h, str(edges.dir / "off.mbias").encode()) == BSX_ERR_STATE
        assert h.L.bsx_meth_set_mbias(h.h, 1) == 0 and fetch() == 0 and cells.sum() == 0 and over.value == 0
        assert h.L.bsx_meth_set_mbias(h.h, 0) == 0 and fetch() == BSX_ERR_STATE   # on, then off again
        h.add(edges.alns[:10], 2)
        assert h.L.bsx_meth_set_mbias(h.h, 1) == BSX_ERR_STATE            # alignments have been added
        assert fetch() == BSX_ERR_STATE
    with handle(edges.fa, mbias=False) as h:
        assert h.L.bsx_meth_set_mbias(h.h, 1) == 0
        h.add(edges.alns[:10], 2)
        assert h.L.bsx_meth_set_mbias(h.h, 0) == BSX_ERR_STATE
        assert h.L.bsx_meth_mbias_fetch(h.h, cells.ctypes.data, C.byref(over)) == 0 and cells.sum() > 0


# ---- 7. command line ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bsp", "sam"])
def test_command_line(fmt, edges, tmp_path, capsys):
    """--mbias and --trim-3p through main(): the file parses back to the cells a handle with the same settings fetches, rows in the
    stated order, NA at depth 0, the comment lines, and the stdout line of a run without --mbias"""
    from bsmap_amd import methratio
    path = str(tmp_path / ("in." + fmt))
    with open(path, "w") as f:
        if fmt == "sam":
            f.write("".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(r)) for n, r in zip(edges.names, edges.refs)))
        for k, (c, pos, st, insert, cut, s) in enumerate(edges.alns):
            if fmt == "sam":  # PNEXT = cut_at + 1; 0 (with a positive insert: "no cut" in the C ABI) where the set has none
                f.write("r%d\t0\t%s\t%d\t255\t%dM\t=\t%d\t%d\t%s\t%s\tNM:i:0\tZS:Z:%s\n" % (k, edges.names[c], pos + 1, len(s), cut + 1, insert, s, "I" * len(s), STRANDS[st]))
            else:
                f.write("r%d\t%s\t%s\tUM\t%s\t%d\t%s\t%d\n" % (k, s, "I" * len(s), edges.names[c], pos + 1, STRANDS[st], insert))
    out, mb = str(tmp_path / "t.txt"), str(tmp_path / "t.mbias")
    methratio.main(["-q", "-z", "-r", "-o", out, "-d", edges.fa, "--mbias", mb, "--trim-3p", "2", path])
    stdout, table = capsys.readouterr().out, open(out).read()
    methratio.main(["-q", "-z", "-r", "-o", out, "-d", edges.fa, "--trim-3p", "2", path])
    assert capsys.readouterr().out == stdout and open(out).read() == table and stdout.startswith("total ")
    cells, over, lmax, rows, comments = parse_mbias(open(mb).read())
    with handle(edges.fa, 1, trim=(0, 2)) as h:
        h.add_file(path)
        got_cells, got_over = h.mbias()
    assert np.array_equal(cells, got_cells) and over == got_over == 0 and cells.sum() > 1000
    # the model on the same alignments (a BSP line carries no mate position: no cut)
    alns = edges.alns if fmt == "sam" else [(c, pos, st, insert, -1, s) for c, pos, st, insert, cut, s in edges.alns]
    assert np.array_equal(cells, model(edges.refs, alns, 2, True, 0, 2)[2])
    # layout: 16 groups in the order strand ++ -+ +- --, context CG CHG CHH CN, each with the cycles 1..Lmax
    assert lmax == max(int(np.nonzero(cells.sum(axis=(0, 1, 3)))[0].max()) + 1, 1) and len(rows) == 16 * lmax
    assert [(r[0], r[1], int(r[2])) for r in rows] == [(s, x, cyc) for s in STRANDS for x in CONTEXTS for cyc in range(1, lmax + 1)]
    assert any(r[5] == "NA" for r in rows) and any(r[5] != "NA" for r in rows)
    assert len(comments) == 5
    for x, line in zip(CONTEXTS, comments):
        m, d = int(cells[:, CONTEXTS.index(x), :, 1].sum()), int(cells[:, CONTEXTS.index(x)].sum())
        assert line == "# total\t%s\t%d\t%d\t%s" % (x, m, d, "NA" if d == 0 else "%.3f" % (float(m) / d))
    assert comments[4] == "# calls beyond cycle 1024: 0"


def test_empty_tally_writes_header_and_comments_only(edges, tmp_path):
    mb = str(tmp_path / "empty.mbias")
    with handle(edges.fa) as h:
        h.write_mbias(mb)
    assert open(mb).read() == "strand\tcontext\tcycle\tmeth\tdepth\tratio\n" + "".join("# total\t%s\t0\t0\tNA\n" % x for x in CONTEXTS) + "# calls beyond cycle 1024: 0\n"
