"""The methylation-ratio tool's file parsers (bsmap_amd/csrc/bsx_meth_parse.h: BSP / SAM lines, BAM records out of BGZF blocks,
the reference FASTA) under AddressSanitizer + UndefinedBehaviorSanitizer, through tests/harness/meth_parse_check.cpp.

Well-formed files: what the parsers hand on must be what oracle/methratio_oracle.py's get_alignment / load_reference (the
restatement of the reference script, pinned by tests/test_methratio_oracle.py) takes from the same text.
Hostile files: the harness must come back with an error or a result — exit status 0, no sanitizer report; an allocation
above 256 MB counts as a report (no header field may size a buffer)."""
import gzip
import json
import os
import random
import struct
import subprocess

import pytest

import bam_util
import golden_util as G
from conftest import HOST_SAN_FLAGS
from oracle import methratio_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio_edges.json.gz"), "rt"))
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mp") / "meth_parse_check")
    subprocess.run(["g++"] + HOST_SAN_FLAGS + ["-o", exe, os.path.join(ROOT, "tests", "harness", "meth_parse_check.cpp"), "-lz"], check=True)   # (ASan + UBSan: conftest.py)
    return exe


def _run(exe, *args, label=""):
    """-> stdout lines; fails on any exit status but 0 (a sanitizer report aborts the harness)"""
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = env.get("ASAN_OPTIONS", "") + ":max_allocation_size_mb=256"
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, timeout=600, env=env)
    assert r.returncode == 0, (label, args, r.returncode, r.stderr.decode(errors="replace")[-3000:])
    return r.stdout.decode("latin-1").split("\n")[:-1]


def _aln(exe, path, fmt, names, unique=0, pair=0, window=256 << 20, piece=256 << 20):
    """-> ([alignment lines], [flush sizes], last line)"""
    out = _run(exe, "aln", path, fmt, ",".join(names), unique, pair, window, piece)
    return [l for l in out[:-1] if not l.startswith("-- flush")], [int(l.split()[2]) for l in out[:-1] if l.startswith("-- flush")], out[-1]


def _expected(text, sam, names, unique=False, pair=False):
    """what get_alignment keeps of every line, trimming and duplicate removal off: (seq after the PNEXT cut, strand[0], chr, pos);
    beside it insert and both strand characters straight from the columns"""
    o = MO.Options(unique=unique, pair=pair, trim_fillin=0)
    exp, nline = [], 0
    for line in text.splitlines(True):
        if sam and line.startswith("@"):
            continue
        nline += 1
        a = MO.get_alignment(line, o, set(names), None, sam)
        if a is None:
            continue
        col = line.rstrip("\n").split("\t")
        strand = [x for x in col[11:] if x[:5] == "ZS:Z:"][0][5:7] if sam else col[6]
        exp.append(a + (int(col[8] if sam else col[7]), strand))
    return exp, nline


def _parsed(lines):
    """harness lines -> the same tuples (the cut is applied the way methratio.py:64 applies it)"""
    out = []
    for l in lines:
        c, pos, strand, insert, cut, seq = l.split("\t")
        pos, cut = int(pos), int(cut)
        out.append((seq[:cut - pos] if cut >= 0 else seq, strand[0], c, pos, int(insert), strand))
    return out


def _names(chroms=None):
    return list(MO.load_reference(EDGES["fasta"], chroms))


def _write(path, text):
    with open(path, "w", newline="", encoding="latin-1") as f:
        f.write(text)
    return str(path)


def _sam_as_bam(sam_text, path, block, rng):
    """the SAM text as BAM (as tests/test_gpu_methratio.py does): optional fields of every type in front of ZS:Z"""
    refs, recs = [], []
    menu = [("XA", "A", "x"), ("Xc", "c", -3), ("XC", "C", 200), ("Xs", "s", -300), ("XS", "S", 60000), ("Xi", "i", -70000), ("XI", "I", 4000000000), ("Xf", "f", 1.5),
            ("XZ", "Z", "some text"), ("XH", "H", "1AE301"), ("Bc", "B", ("c", [-1, 2, 3])), ("BS", "B", ("S", [1, 65535])), ("Bi", "B", ("i", [])), ("Bf", "B", ("f", [0.5, 2.0]))]
    for line in sam_text.splitlines():
        col = line.split("\t")
        if line.startswith("@SQ"):
            refs.append((col[1][3:], int(col[2][3:])))
        if line.startswith("@"):
            continue
        zs = [a for a in col[11:] if a.startswith("ZS:Z:")][0]
        aux = rng.sample(menu, rng.randint(0, len(menu))) + [("ZS", "Z", zs[5:])] + rng.sample(menu, rng.randint(0, 2))
        recs.append(bam_util.mapped_record(col[0], col[9], col[10], int(col[1]), [n for n, _ in refs].index(col[2]), int(col[3]) - 1, int(col[7]) - 1, int(col[8]), aux=aux))
    bam_util.write_bam(path, recs, header_text="".join(l + "\n" for l in sam_text.splitlines() if l.startswith("@")), block=block, refs=refs)
    return str(path)


FILTERS = [(None, 0, 0), (None, 1, 0), (None, 0, 1), (["big", "t4", "k1024"], 1, 1)]


# ---- well-formed files ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["over", "safe", "pairs"])
def test_text_alignments_equal_get_alignment(harness, case, tmp_path):
    fn = EDGES["cases"][case]["infiles"][0]
    text = EDGES["cases"][case]["files"][fn]
    sam = fn.endswith(".sam")
    path = _write(tmp_path / fn, text)
    for chroms, unique, pair in FILTERS:
        names = _names(chroms)
        got, flushes, last = _aln(harness, path, 1 if sam else 0, names, unique, pair)
        exp, nline = _expected(text, sam, names, bool(unique), bool(pair))
        assert _parsed(got) == exp and len(exp) > 100
        assert last == "lines %d" % nline and sum(flushes) == len(exp)


@pytest.mark.parametrize("window", [1, 70000, 256 << 20])
def test_bam_alignments_equal_get_alignment(harness, window, tmp_path):
    """the edge set's SAM case as BAM in 997-byte BGZF blocks: header and records straddle every window edge"""
    text = EDGES["cases"]["pairs"]["files"]["pairs.sam"]
    path = _sam_as_bam(text, tmp_path / "pairs.bam", 997, random.Random(11))
    for chroms, unique, pair in FILTERS:
        names = _names(chroms)
        got, flushes, last = _aln(harness, path, 2, names, unique, pair, window=window)
        exp, nline = _expected(text, True, names, bool(unique), bool(pair))
        assert _parsed(got) == exp and len(exp) > 100
        assert last == "lines %d" % nline
        assert len(flushes) > 50 if window == 1 else len(flushes) >= 1


@pytest.mark.parametrize("case", ["over", "pairs"])
def test_chunks_and_pieces_are_stitched_in_file_order(harness, case, tmp_path):
    """a file above 4 MB: a piece is cut into one chunk per parser thread (1 MB each at least) and the chunks' offset arrays are
    joined; with a 1 MB piece the same file takes several pieces.  Alignments, their order and the line count stay the text's"""
    fn = EDGES["cases"][case]["infiles"][0]
    one = EDGES["cases"][case]["files"][fn]
    sam = fn.endswith(".sam")
    head = "".join(l for l in one.splitlines(True) if sam and l.startswith("@"))
    body = "".join(l for l in one.splitlines(True) if not (sam and l.startswith("@")))
    reps = (5 << 20) // len(body) + 1
    text = head + body * reps
    text = text[:-1]  # no newline after the last line
    path = _write(tmp_path / fn, text)
    assert os.path.getsize(path) > 4 << 20
    names = _names()
    exp, nline = _expected(text, sam, names)
    got, flushes, last = _aln(harness, path, 1 if sam else 0, names)
    assert _parsed(got) == exp and last == "lines %d" % nline and flushes == [len(exp)]
    got, flushes, last = _aln(harness, path, 1 if sam else 0, names, piece=1 << 20)
    assert _parsed(got) == exp and last == "lines %d" % nline and len(flushes) >= 4 and sum(flushes) == len(exp)


FASTAS = {
    "edge_set": lambda: EDGES["fasta"],
    "blank_lines": lambda: ">a\n\nACgt\n\n\nNNac\n>b desc\n\n>c\nGG\n\n",
    "leading_blanks": lambda: ">a\n  ACGT \n\tccgg\t\n >notaheader\nAC\n>  b\tx\n G G \n",
    "name_twice": lambda: ">a\nAAAA\n>b\nCC\n>a\nGGGG\nTT\n>c\nAC\n>b\nT\n",
    "text_before_first_header": lambda: "junk line\nACGT\n>a\nACGT\n>b\nCCGG",
    "crlf_no_final_newline": lambda: ">a one\r\nACGT\r\nacgt\r\n>b\r\nCG",
    "single_letter_records": lambda: ">a\nC\n>b\nG\n>c\n\n>d\nN",
}


@pytest.mark.parametrize("case", sorted(FASTAS))
def test_fasta_records_equal_load_reference(harness, case, tmp_path):
    text = FASTAS[case]()
    path = _write(tmp_path / "g.fa", text)
    for chroms in (None, ["a"], ["b", "big", "t1"], ["t4", "lower", "s03", "k1025"], ["absent"]):
        exp = MO.load_reference(text, chroms)
        out = _run(harness, "fasta", path, ",".join(chroms) if chroms else "-")
        if not exp:
            assert out == ["error 1"]
            continue
        got = [l.split("\t") for l in out]
        assert dict((n, s) for n, s in got) == exp and len(got) == len(exp)
        if case != "name_twice":  # (there the dict keeps the first position, the parser the last record's: the table sorts the names anyway)
            assert [n for n, _ in got] == list(exp)


# ---- hostile files ----------------------------------------------------------------------------------------------------------
def _small_bam_parts(rng, n_rec=40):
    """-> (header bytes, [record bytes], refs): a small mapped BAM whose records carry every optional-field type"""
    refs = [("a", 5000), ("b", 300)]
    menu = [("XA", "A", "x"), ("Xs", "s", -300), ("Xi", "i", 7), ("Xf", "f", 1.5), ("XZ", "Z", "text"), ("XH", "H", "1AE3"), ("Bs", "B", ("s", [1, -2, 3])), ("BC", "B", ("C", [9]))]
    recs = []
    for i in range(n_rec):
        n = rng.randint(1, 120)
        aux = rng.sample(menu, rng.randint(1, 5)) + [("ZS", "Z", rng.choice(["++", "+-", "-+", "--"]))]
        if i == 0:
            aux = [("Bs", "B", ("s", [1, -2, 3]))] + aux
        recs.append(bam_util.mapped_record("q%d" % i, "".join(rng.choice("ACGTN") for _ in range(n)), "I" * n, rng.choice([0, 0x63, 0x93, 0x100]), i % 2, rng.randint(0, 200),
                                           rng.randint(0, 300), rng.choice([0, 150, -150]), aux=aux))
    text = "@HD\tVN:1.0\n@SQ\tSN:a\tLN:5000\n@SQ\tSN:b\tLN:300\n"
    head = b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(refs)) + b"".join(
        struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in refs)
    return head, recs, refs


def _bgzf(data, block):
    return b"".join(bam_util._bgzf_block(data[i:i + block]) for i in range(0, len(data), block)) + bam_util._bgzf_block(b"")


def test_every_prefix_of_a_bam_file(harness, tmp_path):
    """cut off after each of the first 2 000 bytes, then after every 97th: an error or a result, never a read past the prefix"""
    head, recs, _ = _small_bam_parts(random.Random(3))
    raw = _bgzf(head + b"".join(recs), 600)
    assert len(raw) > 3000
    path = str(tmp_path / "small.bam")
    open(path, "wb").write(raw)
    for window in (1, 256 << 20):
        out = _run(harness, "prefixes", path, 2, "a,b", 0, 0, window, 2000, 97)
        assert len(out) == 2000 + (len(raw) - 2000) // 97 + 1
        assert out[0] == "0 error 1" and all(" error 1" in l or " lines " in l for l in out)
        got, _, last = _aln(harness, path, 2, ["a", "b"], window=window)
        assert last == "lines %d" % len(recs) and len(got) > 20


def _mutations():
    """(label, file bytes): one length field of a small BAM file set to 0, -1, INT_MIN, INT_MAX (16-bit fields: to 0, 0xffff, 0x8000,
    0x7fff), in the first block / the header / the first record and again in a later one"""
    head, recs, _ = _small_bam_parts(random.Random(4))
    data = head + b"".join(recs)
    rec_at = [len(head)]
    for r in recs[:-1]:
        rec_at.append(rec_at[-1] + len(r))
    l_text = struct.unpack_from("<i", head, 4)[0]

    def aux_b_count(rec_off):  # record 0 carries a B array as its first optional field: offset of its count
        r = data[rec_off:]
        l_name, n_cig, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<i", r, 20)[0]
        a = rec_off + 36 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        assert data[a:a + 4] == b"BsBs"
        return a + 4
    inflated = {  # name -> (offset in the inflated stream, struct format)
        "l_text": (4, "<i"), "n_ref": (8 + l_text, "<i"), "l_name": (12 + l_text, "<i"),
        "block_size": (rec_at[0], "<i"), "block_size_later": (rec_at[7], "<i"),
        "l_read_name": (rec_at[0] + 12, "<B"), "n_cigar": (rec_at[0] + 16, "<H"), "n_cigar_later": (rec_at[5] + 16, "<H"),
        "l_seq": (rec_at[0] + 20, "<i"), "l_seq_later": (rec_at[9] + 20, "<i"), "B_count": (aux_b_count(rec_at[0]), "<i"),
    }
    for name, (off, fmt) in inflated.items():
        for v in (0, -1, INT_MIN, INT_MAX):
            width = struct.calcsize(fmt)
            patched = bytearray(data)
            patched[off:off + width] = (v & (256 ** width - 1)).to_bytes(width, "little")
            for block in (600, 60000):
                yield "%s=%d/block%d" % (name, v, block), _bgzf(bytes(patched), block)
    raw = _bgzf(data, 600)
    nblk = []
    p = 0
    while p < len(raw):
        nblk.append(p)
        p += struct.unpack_from("<H", raw, p + 16)[0] + 1
    for which, b0 in (("first", nblk[0]), ("middle", nblk[len(nblk) // 2]), ("last", nblk[-1])):
        bsize = struct.unpack_from("<H", raw, b0 + 16)[0] + 1
        for name, off, fmt, values in (("xlen", b0 + 10, "<H", (0, 0xffff, 0x8000, 0x7fff, 4, 5, 7)), ("SLEN", b0 + 14, "<H", (0, 0xffff, 0x8000, 3)),
                                       ("BSIZE", b0 + 16, "<H", (0, 0xffff, 0x8000, 0x7fff, 17, 25)),
                                       ("ISIZE", b0 + bsize - 4, "<I", (0, 0xffffffff, 0x80000000, 0x7fffffff, 65537, 1))):
            for v in values:
                patched = bytearray(raw)
                struct.pack_into(fmt, patched, off, v)
                yield "%s=%d/%s" % (name, v, which), bytes(patched)
    # the extra field as the very last bytes of the file, promising more than there is
    yield "xlen_at_eof", raw + raw[nblk[-1]:nblk[-1] + 18][:10] + struct.pack("<H", 0xffff) + raw[nblk[-1] + 12:nblk[-1] + 18]
    yield "subfields_to_eof", raw + raw[nblk[-1]:nblk[-1] + 10] + struct.pack("<H", 6) + b"XY" + struct.pack("<H", 40) + b"\0\0"


def test_bam_length_fields_set_to_extremes(harness, tmp_path):
    n = 0
    for label, raw in _mutations():
        path = str(tmp_path / "m.bam")
        open(path, "wb").write(raw)
        for window in (1, 256 << 20):
            out = _run(harness, "aln", path, 2, "a,b", 0, 0, window, 256 << 20, label=label)
            assert out and (out[-1].startswith("lines ") or out[-1] in ("error 1", "error 2")), (label, out[-1:])
        n += 1
    assert n > 150


def test_isize_above_the_bgzf_maximum_is_a_format_error(harness, tmp_path):
    head, recs, _ = _small_bam_parts(random.Random(5))
    raw = bytearray(_bgzf(head + b"".join(recs), 600))
    bsize = struct.unpack_from("<H", raw, 16)[0] + 1
    for v in (65537, 1 << 20, INT_MAX, 0xffffffff):
        struct.pack_into("<I", raw, bsize - 4, v)
        path = str(tmp_path / "isize.bam")
        open(path, "wb").write(bytes(raw))
        assert _run(harness, "aln", path, 2, "a,b", 0, 0, 256 << 20, 256 << 20) == ["error 1"]


TEXTS = {  # name -> (format, text, last line expected)
    "empty": (0, "", "lines 0"),
    "empty_sam": (1, "", "lines 0"),
    "only_newlines": (0, "\n\n\n", "lines 3"),
    "too_few_columns": (0, "r1\tACGT\tIIII\n\nr2\tACGT\nr3\tACGT\tIIII\tUM\ta\t5\nr4\tACGT\tIIII\tUM\ta\t5\t+-\n\t\t\t\nr5\tACGT\tIIII\tUM\ta\t5\t++\t0\n", "lines 7"),
    "one_character_strand": (0, "r1\tACGT\tIIII\tUM\ta\t5\t+\t0\n", "error 2"),
    "crlf": (0, "r1\tACGT\tIIII\tUM\ta\t5\t++\t0\t.\t0\r\nr2\tAC\tII\tNM\r\nr3\tACGT\tIIII\tUM\ta\t9\t-+\t12\r\n", "lines 3"),
    "no_final_newline": (0, "r1\tACGT\tIIII\tUM\ta\t5\t++\t0\nr2\tCCGG\tIIII\tMA\tb\t1\t--\t-7", "lines 2"),
    "tabs_only": (0, "\t" * 40, "lines 1"),
    "numbers_that_are_not": (0, "r1\tACGT\tIIII\tUM\ta\tx\t++\ty\nr2\tACGT\tIIII\tUM\ta\t99999999999999999999999\t++\t-99999999999999999999\n", "lines 2"),
    "sam_too_few_columns": (1, "@HD\tVN:1.0\nq1\t0\ta\t5\nq2\n\nq3\t0\ta\t5\t255\t4M\t=\t9\t3\tACGT\n", "lines 4"),
    "sam_without_zs": (1, "@SQ\tSN:a\tLN:99\nq1\t0\ta\t5\t255\t4M\t=\t9\t3\tACGT\tIIII\tNM:i:0\n", "error 2"),
    "sam_without_optional_fields": (1, "q1\t0\ta\t5\t255\t4M\t=\t9\t3\tACGT\tIIII\n", "error 2"),
    "sam_short_zs": (1, "q1\t0\ta\t5\t255\t4M\t=\t9\t3\tACGT\tIIII\tZS:Z:+\n", "error 2"),
    "sam_zs_last_no_newline": (1, "q1\t0\ta\t5\t255\t4M\t=\t9\t3\tACGT\tIIII\tNM:i:0\tZS:Z:-+", "lines 1"),
    "sam_crlf": (1, "@HD\tVN:1.0\r\nq1\t0\ta\t5\t255\t4M\t=\t9\t3\tACGT\tIIII\tZS:Z:+-\r\n", "lines 1"),
    "sam_empty_fields": (1, "q1\t\t\t\t\t\t\t\t\t\t\tZS:Z:++\nq2\t0\tzz\t\t255\t4M\t=\t\t\t\t\tZS:Z:++\n", "lines 2"),
}


@pytest.mark.parametrize("case", sorted(TEXTS))
def test_hostile_text_lines(harness, case, tmp_path):
    fmt, text, last = TEXTS[case]
    path = _write(tmp_path / "t.txt", text)
    for piece in (1, 7, 256 << 20):
        out = _run(harness, "aln", path, fmt, "a,b", 0, 0, 1, piece)
        assert out[-1] == last, (piece, out)
    if last.startswith("lines") and text and "numbers" not in case:  # where get_alignment answers at all, the alignments are its own
        exp = []
        for line in text.splitlines(True):
            if fmt and line.startswith("@"):
                continue
            try:
                a = MO.get_alignment(line, MO.Options(trim_fillin=0), {"a", "b"}, None, bool(fmt))
            except (IndexError, ValueError):
                continue  # (the reference script dies on such a line; the parser skips it)
            if a is not None:
                exp.append(a)
        got, _, _ = _aln(harness, path, fmt, ["a", "b"])
        assert [g[:4] for g in _parsed(got)] == [(s.rstrip("\r\n"), st, c, p) for s, st, c, p in exp]
