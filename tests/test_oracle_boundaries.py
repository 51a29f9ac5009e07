"""The oracle pinned to the REAL reference on directed boundary reads: tests/golden/boundaries_vs_reference.json.gz holds, for every case
below, what the reference's own objects computed on the reads of bsx_testdata.boundary_* — reads built from a position, not drawn: at
letters 0, 1, 2, 15..48 from both ends of every chromosome (29 to 70 001 letters), sticking out of a chromosome, abutting N runs, inside
29- and 30-letter islands, of every length from the seed size to 144 (and 145, 200, which -L cuts), with 0, 1, v and v + 1 placed mismatches,
with f - 1, f and f + 1 N letters, pairs with inserts around -m and -x, RRBS reads from every digestion site with fragments around -m and -x.
The file keeps the same digests as oracle_vs_reference.json.gz (inputs, packed genome and index, a digest per read record, the mapped bits)
and, per read class, how many reads the reference found at their origin.  tests/golden/make_golden_boundaries.py writes it where the
reference is present (each case twice, in two processes, which must agree); the test needs only the repository.  CPU only.

The oracle runs in call order (leak_mode 1), as the reference does: its records must hash to the recorded digests, case by case, and the
first differing read is named."""
import base64
import gzip
import json
import os

import numpy as np
import pytest

import bsx_testdata as td
import test_oracle_vs_reference as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "boundaries_vs_reference.json.gz")

# -s 9 / 12 / 16, -I 1 / 2 / 4 and 8 (no context table above 4), -v 0 / 2 / 6 / 15, -r 0 / 1, -n 0 / 1, a small -w; -f as the class F needs it
SE_CASES = [
    dict(s=16, v=6, I=4, S=1, r=1, n=1, f=5, out_sam=1),
    dict(s=16, v=2, I=4, S=1, r=1, n=0, f=2, out_sam=1),
    dict(s=12, v=0, I=2, S=3, r=1, n=1, f=0, out_sam=1),
    dict(s=9, v=15, I=8, S=3, r=1, n=1, f=5, out_sam=1),
    dict(s=12, v=2, I=1, S=2, r=0, n=1, f=2, w=3, out_sam=1),
    dict(s=16, v=6, I=4, S=7, r=0, n=0, f=5, w=2, out_sam=1),
    dict(s=9, v=2, I=4, S=5, r=1, n=1, f=2, out_sam=1),
]
# -m 0 / 28 / 100, -x 250 / 300 / 500; `length` = the mates' length L of class G
PE_CASES = [
    dict(kw=dict(s=16, v=6, I=4, S=1, r=1, m=28, x=500, out_sam=1), length=50),
    dict(kw=dict(s=16, v=2, I=4, S=1, r=0, m=100, x=300, out_sam=1), length=50),
    dict(kw=dict(s=12, v=2, I=2, S=2, r=1, m=0, x=250, w=4, out_sam=1), length=40),
    dict(kw=dict(s=16, v=0, I=1, S=4, r=1, m=28, x=250, out_sam=1), length=36),
    dict(kw=dict(s=9, v=3, I=4, S=6, r=1, m=28, x=300, out_sam=1), length=50),
]
# the three -D cut positions
RRBS_CASES = [
    dict(D="C-CGG", v=2, S=1, r=1, n=0, m=40, x=220, out_sam=1),
    dict(D="CCG-G", v=4, S=2, r=1, n=1, m=28, x=300, out_sam=1),
    dict(D="-CCGG", v=0, S=3, r=0, n=1, m=100, x=500, out_sam=1),
]
# classes whose reads lie on the far side of a limit: their origin must NOT be in the reference's lists
OUTSIDE = ("Brand", "Bpack", "Eover", "Fover", "Gunder", "Gover", "Hout", "Hend", "Hover")
FLOOR = 8


def _id(kw):
    return "-".join(f"{k}{v}" for k, v in kw.items() if k != "out_sam")


def all_cases():
    """test id -> (kind, case)"""
    out = {}
    for kw in SE_CASES:
        out["test_se[%s]" % _id(kw)] = ("se", dict(kw=kw))
    for c in PE_CASES:
        out["test_pe[%s]" % _id(c["kw"])] = ("pe", c)
    for kw in RRBS_CASES:
        out["test_rrbs[%s]" % _id(kw)] = ("rrbs", dict(kw=kw))
    return out


def case_inputs(kind, case, d):
    """(options, genome, FASTA path written under d, reads) of a case"""
    kw = case["kw"]
    if kind == "rrbs":
        dp = kw["D"].index("-")
        g, sites = td.make_boundary_rrbs_genome(m=kw["m"], x=kw["x"], digest_pos=dp)
        reads = td.boundary_rrbs_reads(g, sites, m=kw["m"], x=kw["x"], v=kw["v"], digest_pos=dp)
        fa = os.path.join(str(d), "rrbs_%s.fa" % kw["D"].replace("-", "_"))
    else:
        g, runs = td.make_boundary_genome()
        fa = os.path.join(str(d), "boundary.fa")
        if kind == "se":
            reads = td.boundary_se_reads(g, runs, s=kw["s"], v=kw["v"], f=kw["f"])
        else:
            reads = td.boundary_pe_reads(g, L=case["length"], m=kw["m"], x=kw["x"])
            kw = dict(kw, pairend=1)
    if not os.path.exists(fa):
        td.write_fasta(fa, g, width=60)
    return kw, g, fa, reads


def origin_found(kind, r, rec):
    """is the read's origin locus in the hit lists (pairs: in the pair lists) of its record (read_record / rrbs_record / pair_record)?"""
    if kind == "pe":
        return any(p[4] >> 1 == r["chr"] and p[6] >> 1 == r["chr"] and {p[5], p[7]} == set(r["locs"]) for w in rec[5] for p in w)
    if rec[0]:
        return False
    return any(h[0] >> 1 == r["chr"] and h[1] == r["pos"] for w in rec[-1] for o in w for h in o)


def class_counts(kind, reads, recs):
    """class -> [reads, reads found at their origin]"""
    out = {}
    for r, rec in zip(reads, recs):
        c = out.setdefault(r["cls"], [0, 0])
        c[0] += 1
        c[1] += bool(origin_found(kind, r, rec[0] if kind == "se" else rec))
    return out


def align_all(kind, kw, reads, al, names, mapped=None):
    """the oracle's record of every read (the same fields make_golden_boundaries.py takes from the reference); mapped[i]: the reference wrote
    a mapped SAM line for single-end read i, whose RNAME / POS / NM / ZS the oracle must reproduce"""
    nclass = kw["v"] + 1
    recs = []
    for i, r in enumerate(reads):
        if kind == "pe":
            recs.append(T.pair_record(al.pe(i, r["seq1"], r["seq2"], r["qual1"], r["qual2"]), al.pe_hits, al.pe_pairs, nclass))
        elif kind == "rrbs":
            recs.append(T.rrbs_record(al.se(i, r["seq"], r["qual"]), al.se_hits, nclass))
        else:
            o = al.se(i, r["seq"], r["qual"])
            recs.append([T.read_record(o, al.se_hits, nclass), T.oracle_sam_fields(o, names) if mapped is not None and mapped[i] else None])
    return recs


@pytest.fixture(scope="module")
def golden():
    return json.load(gzip.open(GOLDEN, "rt"))


def check_case(name, golden, d, oracle):
    kind, case = all_cases()[name]
    gold = golden["cases"][name]
    kw, g, fa, reads = case_inputs(kind, case, d)
    assert T.input_digest(kind, fa, reads) == gold["inputs"], "the directed genome or reads differ from the recorded ones: re-run tests/golden/make_golden_boundaries.py"
    o = oracle.OracleRef(oracle.make_params(**kw), fasta_path=fa)
    assert T.index_digests(kind, kw, T._OracleIndex(o)) == gold["index"]
    al = oracle.OracleAligner(o, leak_mode=1)
    assert gold["n_reads"] == len(reads)
    mapped = np.unpackbits(np.frombuffer(base64.b64decode(gold["sam_mapped"]), np.uint8))[:len(reads)] if kind == "se" else None
    recs = align_all(kind, kw, reads, al, o.names(), mapped)
    al.free()
    o.free()
    digests = [T.record_digest(x) for x in recs]
    total, short = T.summarize_records(digests)
    if total != gold["records"]:
        want = base64.b64decode(gold["read_digest16"])
        bad = [i for i, x in enumerate(digests) if x[:2] != want[2 * i:2 * i + 2]]
        i = bad[0] if bad else None
        raise AssertionError("records differ from the reference's: %s" % ("first at read %d (%s), the oracle's record: %s"
                             % (i, reads[i]["name"], json.dumps(T._json(recs[i]))[:3000]) if bad else "(no single read named)"))
    assert T._json(class_counts(kind, reads, recs)) == gold["classes"]


def check_floors(kind, classes):
    """every class has at least FLOOR reads found at their origin — a class on the far side of a limit at least FLOOR that are NOT (and its
    near side, the rest of its letter, the FLOOR found): what keeps a generator in which nothing maps from passing as agreement"""
    for cls, (n, found) in classes.items():
        if cls in OUTSIDE:
            assert n - found >= FLOOR, (cls, n, found)
        else:
            assert found >= FLOOR, (cls, n, found)
    for letter in {c[0] for c in classes}:
        assert sum(f for c, (n, f) in classes.items() if c[0] == letter) >= FLOOR, letter


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("boundaries")


@pytest.mark.parametrize("kw", SE_CASES, ids=_id)
def test_se(kw, request, golden, workdir, oracle):
    check_case(request.node.name, golden, workdir, oracle)


@pytest.mark.parametrize("case", PE_CASES, ids=lambda c: _id(c["kw"]))
def test_pe(case, request, golden, workdir, oracle):
    check_case(request.node.name, golden, workdir, oracle)


@pytest.mark.parametrize("kw", RRBS_CASES, ids=_id)
def test_rrbs(kw, request, golden, workdir, oracle):
    check_case(request.node.name, golden, workdir, oracle)


def test_recorded_classes_clear_their_floors(golden):
    """the floors the recording script enforced, on what it recorded; and the configurations between them cover what they must"""
    cases = all_cases()
    assert set(golden["cases"]) == set(cases)
    for name, (kind, case) in cases.items():
        check_floors(kind, golden["cases"][name]["classes"])
    se, pe, rr = SE_CASES, [c["kw"] for c in PE_CASES], RRBS_CASES
    assert {9, 12, 16} <= {k["s"] for k in se} and {1, 2, 4} <= {k["I"] for k in se} and any(k["I"] > 4 for k in se)
    assert {0, 2, 6, 15} <= {k["v"] for k in se} and {0, 1} <= {k["r"] for k in se} and {0, 1} <= {k["n"] for k in se} and any(k.get("w", 1000) <= 4 for k in se)
    assert {0, 28, 100} <= {k["m"] for k in pe} and {250, 300, 500} <= {k["x"] for k in pe + rr}
    assert {k["D"] for k in rr} == {"C-CGG", "CCG-G", "-CCGG"}
