#!/usr/bin/env python3
"""Edge-case golden vectors for the methylation-ratio tool (tests/golden/methratio_edges.json.gz).  Build container only.

The fixture of make_golden_methratio.py is real bsmap output on two long chromosomes: depth <= 12, no read near a
chromosome end, no contig shorter than a read.  This one is written by hand (seeded random.Random, no aligner) to sit on
the edges instead, and is answered by the reference's own methratio.py — Python 2, converted with lib2to3 into a
temporary directory at generation time and run with this interpreter; nothing of it is stored.  Stored: the genome
FASTA, the alignment files, option lists, output tables and summary lines, in the format of methratio.json.gz.

  genome  ~30 records: lengths 1..7, 1023, 1024, 1025, 3000, a run of 5-40-letter contigs; a record that ends in C in
          front of one that starts with G; lower-case stretches, N runs, a header with a description, a CRLF record,
          no newline after the last line
  over    BSP lines: starts at 0..3, ends within +-3 of the chromosome end (both sides of the `pos + len > clen` skip),
          lengths 1..160, four strands, flags UM MA OF NM QC (the last two as four-column lines), a name the FASTA
          does not have, inserts around the read length, read letters with N, a tenth of the lines piled on one position
  safe    the same, but every fragment end (methratio.py:53-54) lies inside [0, clen).  The reference script indexes its
          duplicate table with the fragment end unchecked: with -r a '+-' / '-+' read that ends exactly at the chromosome
          end makes it die with IndexError (return code 1) — so -r is asked of this file only.  (The tool under test
          gives such a read no duplicate test; that stays as it is and is not pinned here: a crashed run pins nothing.)
  pairs   SAM lines with @SQ header (read through the vendored samtools, `make -C oracle samtools`): flags with and
          without 0x2, 0x4, 0x100; TLEN > 0 with PNEXT before, inside and behind the read (negative, partial and no cut
          at methratio.py:64); ZS:Z: as the second or third optional field behind fields of other types

The script asserts before it writes: no run crashed; each case's -z table has rows at positions 1 and 2 and at the last two
positions of some chromosome, a depth above 40, and a non-empty context at a position <= 2 (a contig shorter than 5)."""
import gzip
import io
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

STRANDS = ("++", "-+", "+-", "--")
LENGTHS = (1, 2, 3, 30, 63, 64, 65, 100, 128, 129, 150)
TINY_SET = "big,t4,k1024"
OPTION_SETS = [[], ["-z"], ["-t", "0"], ["-t", "1"], ["-t", "200"], ["-g", "-z"], ["-m", "5", "-z"], ["-u", "-p", "-z"], ["-c", TINY_SET]]
SAFE_EXTRA = [["-r", "-z"], ["-r", "-g", "-t", "7", "-z", "-m", "2"]]
N_ALN = 2000


def make_genome(rng):
    """-> [(header text after '>', sequence as written (mixed case), line width, end of line)]"""
    def rnd(n, alphabet="ACGT"):
        return "".join(rng.choice(alphabet) for _ in range(n))

    def dress(s):  # lower-case stretches and N runs
        s = list(s)
        for _ in range(max(1, len(s) // 400)):
            a = rng.randrange(len(s)); b = min(len(s), a + rng.randint(1, 60))
            s[a:b] = [c.lower() for c in s[a:b]]
        for _ in range(len(s) // 700):
            a = rng.randrange(len(s)); b = min(len(s), a + rng.randint(1, 25))
            s[a:b] = ["N"] * (b - a)
        return "".join(s)
    recs = [("t1", "C"), ("t2", "CG"), ("t3", "GCG"), ("t4", "CCGG"), ("t5", "CGCGC"), ("t6", "GCCGGC"), ("t7", "CGACGCG")]
    recs += [("k1023", dress("CG" + rnd(1019, "AACGTT") + "GC")), ("k1024 a description after the name", dress("GC" + rnd(1020, "AACGTT") + "CG")),
             ("k1025\tlength=1025", dress("CCG" + rnd(1019, "AACGTT") + "CGG"))]
    recs.append(("big", dress("CGC" + rnd(2994, "AACGTT") + "GCG")))
    for i in range(12):
        recs.append(("s%02d" % i, "CG" + rnd(rng.randint(1, 36), "ACGTCG") + "GC"))
    recs.append(("endC", rnd(30, "ACGTCG") + "CGC"))
    recs.append(("startG", "GCG" + rnd(30, "ACGTCG")))
    recs.append(("lower", "cg" + rnd(20).lower() + "gc"))
    out = []
    for i, (h, s) in enumerate(recs):
        out.append((h, s, 60 if len(s) > 100 else 7 if i % 3 == 0 else 50, "\r\n" if h == "s03" else "\n"))
    return out


def fasta_text(recs):
    f = io.StringIO()
    for h, s, w, eol in recs:
        f.write(">" + h + eol)
        for a in range(0, len(s), w):
            f.write(s[a:a + w] + eol)
    return f.getvalue().rstrip("\n")  # the last line has no newline


def read_letters(rng, ref, pos, n, strand):
    """bisulfite read of ref[pos:pos+n] on `strand` (random letters past the chromosome's end): C->T ('+') or G->A ('-') on about
    half of the sites, 2 % substitutions, 1 % N"""
    match, conv = ("C", "T") if strand[0] == "+" else ("G", "A")
    out = []
    for k in range(pos, pos + n):
        c = ref[k] if 0 <= k < len(ref) and ref[k] in "ACGT" else rng.choice("ACGT")
        if c == match and rng.random() < 0.55:
            c = conv
        r = rng.random()
        if r < 0.02:
            c = rng.choice("ACGT")
        elif r < 0.03:
            c = "N"
        out.append(c)
    return "".join(out)


def inserts_for(n):
    return [0, 0, 1, -1, 2, -2, 3, n, -n, n + 1, n + 2, -(n + 2), n + 3, 250, -250, n // 2, -(n // 2)]


def placements(rng, ref, names, n_aln, safe):
    """-> [(chr, pos, length, strand)]: whole tiny contigs on every strand first, then the seeded edge mix"""
    out = []
    for c in names:
        if len(ref[c]) <= 7 or c in ("s00", "lower", "endC", "startG"):
            for st in STRANDS:
                for _ in range(3):
                    out.append((c, 0, len(ref[c]), st))
    pile_chr, pile_pos, pile_len = "big", 1500, 100
    while len(out) < n_aln:
        if rng.random() < 0.10:
            out.append((pile_chr, pile_pos, pile_len, rng.choice(STRANDS)))
            continue
        c = rng.choice(names) if rng.random() < 0.5 else rng.choice(["big", "k1023", "k1024", "k1025"])
        clen = len(ref[c])
        n = rng.choice(LENGTHS) if rng.random() < 0.6 else rng.randint(1, 160)
        kind = rng.random()
        if kind < 0.25:
            pos = rng.randint(0, 3)
        elif kind < 0.60:
            pos = clen + rng.randint(-3, 3) - n
        else:
            pos = rng.randint(0, max(0, clen - n))
        pos = max(0, pos)
        out.append((c, pos, n, rng.choice(STRANDS)))
    if safe:  # every fragment end inside [0, clen): the read's right end for '+-' / '-+', its left end otherwise
        fixed = []
        for c, pos, n, st in out:
            clen = len(ref[c])
            if st in ("+-", "-+"):
                n = min(n, clen - 1)
                pos = min(pos, clen - 1 - n)
                if n < 1:
                    continue  # (a one-letter contig holds no such read)
            else:
                pos = min(pos, clen - 1)
            fixed.append((c, pos, n, st))
        out = fixed
    return out


def bsp_lines(rng, ref, names, n_aln, safe):
    lines = []
    for i, (c, pos, n, st) in enumerate(placements(rng, ref, names, n_aln, safe)):
        seq = read_letters(rng, ref[c], pos, n, st)
        r = rng.random()
        flag = "UM" if r < 0.62 else "MA" if r < 0.74 else "OF" if r < 0.84 else "NM" if r < 0.92 else "QC"
        if flag in ("NM", "QC"):
            lines.append("r%d\t%s\t%s\t%s\n" % (i, seq, "I" * n, flag))
            continue
        if rng.random() < 0.02:
            c = "ghost"  # a name the FASTA does not have
        ins = rng.choice(inserts_for(n)) if len(ref.get(c, "")) > 7 or rng.random() < 0.5 else 0
        lines.append("r%d\t%s\t%s\t%s\t%s\t%d\t%s\t%d\t.\t0\t0:0:0:0:0\n" % (i, seq, "I" * n, flag, c, pos + 1, st, ins))
    return "".join(lines)


def sam_text(rng, ref, names, n_aln):
    out = ["@HD\tVN:1.0\tSO:unsorted\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (c, len(ref[c])) for c in names]
    front = [[], ["NM:i:1"], ["XA:A:x", "XF:f:1.5"], ["XZ:Z:some text", "NM:i:0"], ["XH:H:1AE301"]]
    for i, (c, pos, n, st) in enumerate(placements(rng, ref, names, n_aln, True)):
        seq = read_letters(rng, ref[c], pos, n, st)
        flag = rng.choice([0x1, 0x1 | 0x2, 0x1 | 0x2, 0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80 | 0x20, 0x1 | 0x2 | 0x100, 0x100, 0x4, 0x1 | 0x4 | 0x8, 0x10, 0])
        tiny = len(ref[c]) <= 7
        r = rng.random()
        if tiny and r < 0.6:
            tlen, pnext = 0, pos + 1
        elif r < 0.30:
            tlen, pnext = rng.choice([1, 2, 3, n, n + 1, n + 3, 250, n // 2 + 1]), max(1, pos + 1 - rng.randint(1, 5))      # before the read: negative cut
        elif r < 0.60:
            tlen, pnext = rng.choice([1, 3, n, n + 2, 250, n // 2 + 1]), pos + 1 + rng.randint(0, n)                         # inside: partial cut
        elif r < 0.75:
            tlen, pnext = rng.choice([n + 3, 250, 400]), pos + 1 + n + rng.randint(0, 200)                                  # behind: no cut
        else:
            tlen, pnext = rng.choice([0, -1, -2, -n, -(n + 2), -250, -(n // 2)]), max(1, pos + 1 - rng.randint(0, 200))
        opt = list(rng.choice(front)) + ["ZS:Z:" + st] + (["XT:i:7"] if rng.random() < 0.3 else [])
        out.append("p%d\t%d\t%s\t%d\t255\t%dM\t=\t%d\t%d\t%s\t%s\t%s\n" % (i, flag, c, pos + 1, n, pnext, tlen, seq, "I" * n, "\t".join(opt)))
    return "".join(out)


def check_case(name, ref, case):
    assert not any(r["crashed"] for r in case["runs"]), (name, [r["options"] for r in case["runs"] if r["crashed"]])
    table = [r for r in case["runs"] if r["options"] == ["-z"]][0]["table"]
    rows = [l.split("\t") for l in table.split("\n")[1:] if l]
    at = {}
    for f in rows:
        at.setdefault(f[0], set()).add(int(f[1]))
    assert any({1, 2} <= s for s in at.values()), name
    assert any({len(ref[c]) - 1, len(ref[c])} <= s for c, s in at.items()), name
    assert max(int(f[5]) for f in rows) > 40, name
    assert any(int(f[1]) <= 2 and f[3] != "" and len(ref[f[0]]) < 5 for f in rows), name


def main():
    from oracle import methratio_oracle as MO
    from oracle import ref_ffi as R
    tmp = tempfile.mkdtemp()
    conv = os.path.join(tmp, "conv")
    os.makedirs(conv)
    shutil.copy(os.path.join(R.REFERENCE_DIR, "methratio.py"), conv)
    subprocess.run([sys.executable, "-m", "lib2to3", "-w", "-n", os.path.join(conv, "methratio.py")], check=True, capture_output=True)
    script = os.path.join(conv, "methratio.py")
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "samtools"], check=True, capture_output=True)
    sam_dir = os.path.join(ROOT, "oracle", "_ref")

    rng = random.Random(20240611)
    fasta = fasta_text(make_genome(rng))
    fa = os.path.join(tmp, "g.fa")
    with open(fa, "w", newline="") as f:
        f.write(fasta)
    ref = MO.load_reference(fasta)
    names = list(ref)
    cases = {
        "over": dict(files={"over.bsp": bsp_lines(random.Random(1), ref, names, N_ALN, False)}, infiles=["over.bsp"], option_sets=OPTION_SETS),
        "safe": dict(files={"safe.bsp": bsp_lines(random.Random(2), ref, names, N_ALN, True)}, infiles=["safe.bsp"], option_sets=OPTION_SETS + SAFE_EXTRA),
        "pairs": dict(files={"pairs.sam": sam_text(random.Random(3), ref, names, N_ALN)}, infiles=["pairs.sam"], option_sets=OPTION_SETS),
    }
    for name, c in cases.items():
        d = os.path.join(tmp, name); os.makedirs(d)
        for fn, txt in c["files"].items():
            open(os.path.join(d, fn), "w").write(txt)
        c["runs"] = []
        for opts in c.pop("option_sets"):
            out = os.path.join(d, "out.txt")
            sam_opt = ["-s", sam_dir] if name == "pairs" else []
            res = subprocess.run([sys.executable, script, "-q", "-o", out, "-d", fa] + sam_opt + opts + [os.path.join(d, f) for f in c["infiles"]],
                                 capture_output=True, text=True)
            c["runs"].append(dict(options=opts, table=open(out).read(), stdout=res.stdout, crashed=res.returncode != 0))
        check_case(name, ref, c)
        print(name, {" ".join(r["options"]) or "-": r["table"].count("\n") for r in c["runs"]}, c["runs"][0]["stdout"].strip())
    path = os.path.join(HERE, "methratio_edges.json.gz")
    with open(path, "wb") as raw:  # (no file name, no time stamp in the gzip header: the file regenerates byte for byte)
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as gz:
            gz.write(json.dumps(dict(fasta=fasta, cases=cases), sort_keys=True).encode())
    print(path, os.path.getsize(path), "bytes")
    shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
