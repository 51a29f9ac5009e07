"""Pinning of the oracle against the REAL reference objects, through their recorded answers: tests/golden/oracle_vs_reference.json.gz
holds, for every case below, what oracle/_ref/libbsmapref.so (the reference's own objects behind oracle/ref_harness.cpp) computed on
the same seeded genomes and reads, as digests: of the packed genome and seed index, and of the record of every read (planner state, every
hit list, every pair list, the fields of a mapped SAM line) — the oracle's records must hash to the same.  tests/golden/make_golden_vs_reference.py writes it where the reference is present; the test itself needs only the
repository.  CPU only."""
import base64
import gzip
import hashlib
import json
import os
import random

import numpy as np
import pytest

import bsx_testdata as td

ADAPTER = "AGATCGGAAGAGC"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vs_reference.json.gz")


def _digest(a):
    a = np.asarray(a)
    return hashlib.sha256(repr(a.shape).encode() + a.astype(np.int64).tobytes()).hexdigest()[:32]


def _text_digest(x):
    return hashlib.sha256(json.dumps(x, sort_keys=True).encode()).hexdigest()[:32]


def make_genomes(d):
    """the two genomes every case runs on, written as FASTA files under d: (WGBS genome, its path, RRBS genome, its path)"""
    g = td.make_genome(seed=1, chr_lens=(200_000, 90_000, 30_017), gc=0.51)
    fa = os.path.join(str(d), "g.fa")
    td.write_fasta(fa, g)
    gr = td.make_genome(seed=4, chr_lens=(250_000, 80_000), gc=0.55, cpg_sites=1200)
    far = os.path.join(str(d), "gr.fa")
    td.write_fasta(far, gr)
    return g, fa, gr, far


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    return make_genomes(tmp_path_factory.mktemp("ref"))


@pytest.fixture(scope="module")
def golden():
    return json.load(gzip.open(GOLDEN, "rt"))


# ---- the record of one read: the fields the reference and the oracle must agree on, the same for both sides ----------------------------

def read_record(st, hits, nclass):
    """planner state (the seed arrays only for a chain that exists), per-class hit counts and every hit list; nothing past `filtered`
    for a filtered read"""
    rec = [st.filtered, st.len, st.raw_len]
    if st.filtered:
        return rec
    n = st.seedseg_num
    rec += [st.read_max_snp_num, n, st.flag_chain, st.cflag_chain, st.snp_thres,
            [list(st.seed_start_array)[:n], list(st.seedindex)[:n], list(st.seedcount)[:n]] if st.flag_chain else None,
            [list(st.cseed_start_array)[:n], list(st.cseedindex)[:n]] if st.cflag_chain else None,
            list(st.n_hit)[:nclass], list(st.n_chit)[:nclass],
            [[[list(h) for h in hits(orient, w, (st.n_chit if orient else st.n_hit)[w])] for orient in (0, 1)] for w in range(nclass)]]
    return rec


def rrbs_record(st, hits, nclass):
    rec = [st.filtered, st.len]
    if st.filtered:
        return rec
    return rec + [list(st.n_hit)[:nclass], list(st.n_chit)[:nclass],
                  [[[list(h) for h in hits(orient, w, (st.n_chit if orient else st.n_hit)[w])] for orient in (0, 1)] for w in range(nclass)]]


def pair_record(st, hits, pairs, nclass):
    """hits(mate, orient, w, n), pairs(w, n)"""
    return [st.paired, st.tmp, list(st.n_pairs),
            read_record(st.a, lambda o, w, n: hits(0, o, w, n), nclass), read_record(st.b, lambda o, w, n: hits(1, o, w, n), nclass),
            [[list(p) for p in pairs(w, st.n_pairs[w])] for w in range(2 * nclass - 1)]]


def sam_fields(line):
    """what a mapped SAM line of the reference is checked on: RNAME, POS, the NM tag and the ZS strand tag"""
    f = line.split("\t")
    if not line or f[2] == "*":
        return None
    zs = [t for t in f if t.startswith("ZS:Z:")]
    return [f[2], int(f[3]), f[11], zs[0][:7] if zs else None]


def oracle_sam_fields(o, names):
    return [names[o.chr >> 1], o.loc + 1, "NM:i:%d" % o.best_class, "ZS:Z:" + "+-"[o.chr & 1] + "+-"[o.chain]]


# ---- the cases ---------------------------------------------------------------------------------------------------------------

SE_CASES = [
    dict(kw=dict(s=12, v=2, I=4, S=1, r=1, out_sam=1), length=36, sub=0.02, strands=("++", "-+")),
    dict(kw=dict(s=16, v=4, I=4, S=1, r=1, n=1, out_sam=1), length=100, sub=0.01),
    dict(kw=dict(s=16, v=4, I=4, S=7, r=0, n=0, out_sam=1), length=100, sub=0.01),
    dict(kw=dict(s=16, v=6, I=4, S=3, r=1, n=1, out_sam=1, q=20, A=[ADAPTER]), length=144, sub=0.01, var=True, trim=True),
    dict(kw=dict(s=14, v=5, I=2, S=3, r=1, n=1, out_sam=1, w=5), length=144, sub=0.01, var=True),
    dict(kw=dict(s=10, v=3, I=1, S=3, r=0, n=1, out_sam=1, w=3), length=144, sub=0.01, var=True),
    dict(kw=dict(s=9, v=15, I=16, S=3, r=1, n=1, out_sam=0, w=1000, M="GA"), length=80, sub=0.02, n=300),
]
PE_CASES = [
    dict(kw=dict(s=16, v=6, I=4, S=1, r=1, m=28, x=500, out_sam=1), length=150),
    dict(kw=dict(s=16, v=6, I=4, S=1, r=0, m=28, x=500, out_sam=1), length=150),
    dict(kw=dict(s=16, v=6, I=4, S=1, r=1, m=28, x=500, out_sam=1, q=20, A=[ADAPTER]), length=150, trim=True),
    dict(kw=dict(s=12, v=3, I=2, S=2, r=1, n=1, m=0, x=300, out_sam=1, w=4), length=150, trim=True),
]
RRBS_KW = [dict(D="C-CGG", v=4, S=1, r=1, out_sam=1), dict(D="C-CGG", v=2, S=1, r=0, n=1, out_sam=1, A=[ADAPTER])]
RRBS_IDS = ["rrbs-v4", "rrbs-n1-r0"]
QUALS = [5, 20]
SE_SEEDS = list(range(301, 333))
PE_SEEDS = list(range(401, 421))
RRBS_SEEDS = list(range(501, 515))


def _case_id(c):
    return "-".join(f"{k}{v}" for k, v in c["kw"].items() if k not in ("A", "out_sam"))


def _random_case(seed):
    """a seeded draw from the option space of the command line (main.cpp:234-289) — the same space the GPU path is
    fuzzed over in tests/test_gpu_parity.py"""
    rng = random.Random(seed)
    kw = dict(s=rng.randint(9, 16), v=rng.choice([0, 1, 2, 3, 4, 5, 6, 8, 11]), I=rng.choice([1, 2, 3, 4, 4, 5, 8]), S=rng.randint(1, 99),
              r=rng.choice([0, 1, 1]), n=rng.choice([0, 1]), w=rng.choice([1, 2, 7, 50, 1000]), f=rng.choice([0, 2, 5]),
              L=rng.choice([144, 144, 100, 61]), out_sam=1)
    if rng.random() < 0.3:
        kw["M"] = rng.choice(["GA", "CT", "AG", "TG"])
    trim = rng.random() < 0.4
    if trim:
        kw.update(q=rng.choice([5, 20, 30]), A=[ADAPTER])
    return kw, trim, rng


def _quality_reads(g):
    """a malformed FASTQ record may carry more or fewer quality characters than bases"""
    rng = np.random.default_rng(5)
    reads = td.make_se_reads(g, 120, 60, seed=9, sub_rate=0.004, strands=("++", "-+"))
    for i, r in enumerate(reads):
        L = len(r["seq"])
        tail = "".join(chr(int(x)) for x in rng.integers(35, 49, 30))
        if i % 3 == 0:
            r["qual"] = "I" * (L - 25) + tail[:25] + tail            # longer than the read, low tail with a few good characters beyond it
        elif i % 3 == 1:
            r["qual"] = "I" * (L - 20)                               # shorter than the read
        else:
            r["qual"] = "I" * (L - 30) + tail                        # same length, low tail
    return reads


def all_cases():
    """test id -> (kind, case): every case of this module, under the name of the test that runs it"""
    out = {}
    for c in SE_CASES:
        out["test_se[%s]" % _case_id(c)] = ("se", c)
    for c in PE_CASES:
        out["test_pe[%s]" % _case_id(c)] = ("pe", c)
    for kw, i in zip(RRBS_KW, RRBS_IDS):
        out["test_rrbs[%s]" % i] = ("rrbs", dict(kw=kw))
    for q in QUALS:
        out["test_quality_string_longer_or_shorter_than_the_read[%d]" % q] = ("se", dict(kw=dict(s=14, v=4, I=1, S=54, r=0, n=1, w=50, out_sam=1, q=q), quality=True))
    for seed in SE_SEEDS:
        kw, trim, rng = _random_case(seed)
        out["test_se_random_options[%d]" % seed] = ("se", dict(kw=kw, length=rng.choice([150, 120, 80, 40]), sub=0.006, var=rng.random() < 0.5, trim=trim, n=500))
    for seed in PE_SEEDS:
        kw, trim, rng = _random_case(seed)
        kw.pop("n")
        kw.update(m=rng.choice([0, 28, 120]), x=rng.choice([250, 500, 900]))
        out["test_pe_random_options[%d]" % seed] = ("pe", dict(kw=kw, length=rng.choice([150, 120, 80]), trim=trim))
    for seed in RRBS_SEEDS:
        rng = random.Random(seed)
        kw = dict(D=rng.choice(["C-CGG", "C-CGG", "CCG-G", "-CCGG"]), v=rng.choice([0, 1, 2, 3, 5]), S=rng.randint(1, 90), r=rng.choice([0, 1, 1]),
                  w=rng.choice([1, 3, 100, 1000]), m=rng.choice([20, 40, 80]), x=rng.choice([150, 220, 400]), L=rng.choice([144, 75, 50]),
                  n=rng.choice([0, 1]), out_sam=1)
        out["test_rrbs_random_options[%d]" % seed] = ("rrbs", dict(kw=kw))
    return out


def case_inputs(kind, case, genome):
    """(options, fasta path, reads) of a case"""
    g, fa, gr, far = genome
    if kind == "se":
        if case.get("quality"):
            return case["kw"], fa, _quality_reads(g)
        reads = td.make_se_reads(g, case.get("n", 1500), case["length"], seed=2, sub_rate=case["sub"], var_len=case.get("var", False),
                                 strands=case.get("strands", ("++", "-+", "+-", "--")), qual_tail=case.get("trim", False),
                                 adapter=ADAPTER if case.get("trim") else None)
        return case["kw"], fa, reads
    if kind == "pe":
        trim = case.get("trim", False)
        pairs = td.make_pe_reads(g, 1000, case["length"], seed=6, sub_rate=0.015, qual_tail=trim, adapter=ADAPTER if trim else None,
                                 var_len=trim, ins_min=20 if trim else 50, ins_mean=200 if trim else 300, ins_sd=100 if trim else 50)
        return dict(case["kw"], pairend=1), fa, pairs
    reads = td.make_rrbs_reads(gr, 1200, 75, seed=3) + td.make_se_reads(gr, 200, 75, seed=9, var_len=True)
    return case["kw"], far, reads


def input_digest(kind, fa, reads):
    keys = ("name", "seq1", "qual1", "seq2", "qual2") if kind == "pe" else ("name", "seq", "qual")
    return _text_digest([open(fa).read(), [[r[k] for k in keys] for r in reads]])


def index_digests(kind, kw, ref):
    """digests of the reference's (or the oracle's) packed genome and seed index: `ref` answers refcat/crefcat/blocks/anchor and csr(),
    or rrbs_csr() and sites(c).  (The paired-end cases check reads and pairs only.)"""
    if kind == "pe":
        return {}
    if kind == "rrbs":
        off, ent = ref.rrbs_csr()
        return {"bucket_off": _digest(off), "rrbs_entries": _digest(ent), "sites0": _digest(ref.sites(0)), "sites1": _digest(ref.sites(1))}
    d = {"refcat": _digest(ref.refcat()[400:-400]), "crefcat": _digest(ref.crefcat()[400:-400]), "blocks": _digest(ref.blocks()), "anchor": _digest(ref.anchor())}
    if kw["s"] <= 12:
        off, nf, ent = ref.csr()
        d.update(bucket_off=_digest(off), bucket_nfwd=_digest(nf), entries=_digest(ent))
    return d


class _OracleIndex:
    """the oracle's reference in the shape index_digests() reads"""
    def __init__(self, o):
        self.o = o
        self.refcat, self.crefcat, self.blocks, self.anchor, self.sites = o.refcat, o.crefcat, o.blocks, o.anchor, o.sites

    def csr(self):
        return self.o.bucket_off(), self.o.bucket_nfwd(), self.o.entries()

    def rrbs_csr(self):
        return self.o.bucket_off(), self.o.rrbs_entries()


def _json(x):
    return json.loads(json.dumps(x))


def record_digest(rec):
    return hashlib.sha256(json.dumps(_json(rec), separators=(",", ":")).encode()).digest()


def summarize_records(digests):
    """what the golden file keeps of a case's read records: the SHA-256 over every read's record digest in read order (the check), and
    the first two bytes of each read's digest (base64; only to name the first read that differs)"""
    return hashlib.sha256(b"".join(digests)).hexdigest(), base64.b64encode(b"".join(d[:2] for d in digests)).decode()


def check_case(name, golden, genome, oracle):
    kind, case = all_cases()[name]
    gold = golden["cases"][name]
    kw, fa, reads = case_inputs(kind, case, genome)
    assert input_digest(kind, fa, reads) == gold["inputs"], "the seeded genome or reads differ from the recorded ones: re-run tests/golden/make_golden_vs_reference.py"
    o = oracle.OracleRef(oracle.make_params(**kw), fasta_path=fa)
    assert index_digests(kind, kw, _OracleIndex(o)) == gold["index"]
    al = oracle.OracleAligner(o, leak_mode=1)
    nclass = kw["v"] + 1
    names = o.names()
    assert gold["n_reads"] == len(reads)
    # SE: the reads whose SAM line the reference mapped, the ones whose RNAME / POS / NM / ZS the oracle must reproduce
    mapped = np.unpackbits(np.frombuffer(base64.b64decode(gold["sam_mapped"]), np.uint8))[:len(reads)] if kind == "se" else None
    recs = []
    for i, r in enumerate(reads):
        if kind == "pe":
            os_ = al.pe(i, r["seq1"], r["seq2"], r["qual1"], r["qual2"])
            recs.append(pair_record(os_, al.pe_hits, al.pe_pairs, nclass))
        elif kind == "rrbs":
            recs.append(rrbs_record(al.se(i, r["seq"], r["qual"]), al.se_hits, nclass))
        else:
            os_ = al.se(i, r["seq"], r["qual"])
            recs.append([read_record(os_, al.se_hits, nclass), oracle_sam_fields(os_, names) if mapped[i] else None])
    al.free()
    o.free()
    digests = [record_digest(x) for x in recs]
    total, short = summarize_records(digests)
    if total != gold["records"]:
        want = base64.b64decode(gold["read_digest16"])
        bad = [i for i, d in enumerate(digests) if d[:2] != want[2 * i:2 * i + 2]]
        i = bad[0] if bad else None
        raise AssertionError("records differ from the reference's: %s" % ("first at read %d (%s), the oracle's record: %s"
                             % (i, reads[i]["name"], json.dumps(_json(recs[i]))[:3000]) if bad else "(no single read named)"))


@pytest.mark.parametrize("case", SE_CASES, ids=_case_id)
def test_se(case, request, golden, genome, oracle):
    check_case(request.node.name, golden, genome, oracle)


@pytest.mark.parametrize("case", PE_CASES, ids=_case_id)
def test_pe(case, request, golden, genome, oracle):
    check_case(request.node.name, golden, genome, oracle)


@pytest.mark.parametrize("kw", RRBS_KW, ids=RRBS_IDS)
def test_rrbs(kw, request, golden, genome, oracle):
    check_case(request.node.name, golden, genome, oracle)


@pytest.mark.parametrize("q", QUALS)
def test_quality_string_longer_or_shorter_than_the_read(q, request, golden, genome, oracle):
    """a malformed FASTQ record may carry more or fewer quality characters than bases: the reference keeps both lengths, and its
    TrimLowQual scans the whole quality string (align.cpp:69-78) — a good character beyond the last base keeps the read untrimmed, a
    short string cuts the read to its length.  (At the C ABI a batch has one offset array for bases and qualities, so the device path
    never sees such a record; the command line cuts or pads the quality string to the read)"""
    check_case(request.node.name, golden, genome, oracle)


@pytest.mark.parametrize("seed", SE_SEEDS)
def test_se_random_options(seed, request, golden, genome, oracle):
    check_case(request.node.name, golden, genome, oracle)


@pytest.mark.parametrize("seed", PE_SEEDS)
def test_pe_random_options(seed, request, golden, genome, oracle):
    check_case(request.node.name, golden, genome, oracle)


@pytest.mark.parametrize("seed", RRBS_SEEDS)
def test_rrbs_random_options(seed, request, golden, genome, oracle):
    check_case(request.node.name, golden, genome, oracle)
