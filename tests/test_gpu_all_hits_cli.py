"""bsmap --all-hits=FILE on the golden CLI inputs.  Needs an MI355X.
  * the main output with the option is byte-identical to the one without (which test_gpu_cli.py holds to the reference binary's);
  * the side file's lines, mapped back through chromosome names and strands, equal the oracle's best-class lists of every unit, in input order;
  * the line whose k is the reported pick repeats RNAME, POS and ZS:Z of the unit's primary SAM line(s);
  * a starting pool that is too small (BSX_ALL_HITS_POOL) is grown and the batch run again: same side file, one line on stderr;
  * --lanes=2 gives the same side file as one pipeline; --lane-files leaves FILE.<lane>."""
import gzip
import json
import os
import subprocess

import pytest

import golden_util as G
from test_gpu_all_hits import EMITTING, myrand, oracle_pe_lists, oracle_se_lists

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bsmap_amd", "bsmap")
CLI = json.load(gzip.open(os.path.join(G.GOLDEN, "cli_outputs.json.gz"), "rt"))
NAMES = [n for n in sorted(CLI) if n in EMITTING]


def _inputs(meta, tmp_path):
    if meta["kind"] == "pe":
        f1, f2 = str(tmp_path / "r_1.fq"), str(tmp_path / "r_2.fq")
        with open(f1, "w") as a, open(f2, "w") as b:
            for r in meta["reads"]:
                a.write(f"@{r['name']}/1\n{r['seq1']}\n+\n{r['qual1']}\n")
                b.write(f"@{r['name']}/2\n{r['seq2']}\n+\n{r['qual2']}\n")
        return ["-a", f1, "-b", f2]
    f1 = str(tmp_path / "r.fq")
    with open(f1, "w") as a:
        for r in meta["reads"]:
            a.write(f"@{r['name']}\n{r['seq']}\n+\n{r['qual']}\n")
    return ["-a", f1]


def _run(meta, fasta, inputs, out, extra, env=None):
    opts = list(CLI[meta["config"]]["sam_plain"]["options"])
    cmd = [BIN] + inputs + ["-d", fasta, "-o", out] + opts + extra
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-1500:]
    return res


def _side(path):
    lines = open(path).read().split("\n")
    assert lines[0].startswith("#name\tkind\tk\tn\tchr\tpos\tstrand\tmismatches") and lines[-1] == ""
    return [l.split("\t") for l in lines[1:-1]]


def _expected_lines(meta, oracle, oref, names):
    """the side file the oracle's lists give: one tuple of fields per line, in input order; also {read name: (kind, picked line)}"""
    kw = meta["kw"]
    S = kw.get("S", 0)
    al = oracle.OracleAligner(oref, leak_mode=0)
    st = lambda chr_, chain: "+-"[chr_ % 2] + "+-"[chain]
    want, picks = [], {}
    for i, r in enumerate(meta["reads"]):
        if meta["kind"] == "se":
            o = al.se(i, r["seq"], r["qual"])
            hits = oracle_se_lists(al, o)[0]
            nf = o.n_hit[o.best_class] if hits else 0
            rows = [(r["name"], "0", str(k), str(len(hits)), names[c >> 1], str(l + 1), st(c, int(k >= nf)), str(o.best_class)) for k, (c, l) in enumerate(hits)]
            if rows:
                picks[r["name"]] = [rows[myrand(i, S) % len(rows)]]
            want += rows
            continue
        o = al.pe(i, r["seq1"], r["seq2"], r["qual1"], r["qual2"])
        la, lb, lp = oracle_pe_lists(al, o)
        for kind, om, hits in ((1, o.a, la), (2, o.b, lb)):
            nf = om.n_hit[om.best_class] if hits else 0
            rows = [(r["name"], str(kind), str(k), str(len(hits)), names[c >> 1], str(l + 1), st(c, int(k >= nf)), str(om.best_class)) for k, (c, l) in enumerate(hits)]
            if rows:
                picks.setdefault(r["name"], []).append(rows[myrand(i, S) % len(rows)])
            want += rows
        rows = []
        for k, (chain, na, nb, ins, ac, a_loc, bc, b_loc) in enumerate(lp):
            if ins < o.a.len and (chain ^ (ac % 2)):      # s_OutHitPair's cut of a read-through (pairs.cpp:296-311)
                a_loc += o.a.len - ins
            if ins < o.b.len and ((1 - chain) ^ (bc % 2)):
                b_loc += o.b.len - ins
            assert ac >> 1 == bc >> 1
            rows.append((r["name"], "P", str(k), str(len(lp)), names[ac >> 1], str(a_loc + 1), st(ac, chain), str(b_loc + 1), st(bc, 1 - chain), str(ins), str(na), str(nb)))
        if rows:
            picks[r["name"]] = [rows[myrand(i, S) % len(rows)]]
        want += rows
    al.free()
    return want, picks


def _sam_primary(path):
    """{read name: {mate (0 single, 1, 2): (RNAME, POS, ZS)}} of the mapped lines"""
    out = {}
    for l in open(path):
        if l.startswith("@"):
            continue
        f = l.rstrip("\n").split("\t")
        flag = int(f[1])
        if flag & 0x4:
            continue
        zs = [x[5:] for x in f[11:] if x.startswith("ZS:Z:")][0]
        out.setdefault(f[0], {})[1 if flag & 0x40 else 2 if flag & 0x80 else 0] = (f[2], f[3], zs)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_side_file_equals_the_oracles_lists_and_main_output_is_untouched(name, oracle, tmp_path):
    meta, arr, fasta = G.load(name)
    inputs = _inputs(meta, tmp_path)
    plain, with_, side = str(tmp_path / "plain.sam"), str(tmp_path / "with.sam"), str(tmp_path / "all.tsv")
    _run(meta, fasta, inputs, plain, [])
    res = _run(meta, fasta, inputs, with_, [f"--all-hits={side}"])
    assert open(plain, "rb").read() == open(with_, "rb").read() and "pool grown" not in res.stderr
    oref = oracle.OracleRef(oracle.make_params(**meta["kw"]), fasta_path=fasta)
    try:
        want, picks = _expected_lines(meta, oracle, oref, oref.names())
    finally:
        oref.free()
    got = [tuple(f) for f in _side(side)]
    assert got == want
    assert len({f[0] for f in got}) == EMITTING[name][0]
    # the picked line repeats the primary line's RNAME, POS and ZS:Z
    sam = _sam_primary(with_)
    for nm, rows in picks.items():
        for row in rows:
            if row[1] == "P":
                assert sam[nm][1] == (row[4], row[5], row[6]) and sam[nm][2] == (row[4], row[7], row[8]), nm
            else:
                assert sam[nm][int(row[1])] == (row[4], row[5], row[6]), nm
    # a pool that is too small is grown and the batch run again before anything is formatted; many small batches on five workers: the same bytes
    side2 = str(tmp_path / "all2.tsv")
    res = _run(meta, fasta, inputs, str(tmp_path / "w2.sam"), [f"--all-hits={side2}", "-p", "5"], {"BSX_ALL_HITS_POOL": "64", "BSX_BATCH": "97"})
    assert open(side2, "rb").read() == open(side, "rb").read() and open(str(tmp_path / "w2.sam"), "rb").read() == open(plain, "rb").read()
    if EMITTING[name][1] * 2 > 64:
        assert "pool grown, batch run again" in res.stderr


@pytest.mark.parametrize("name", ["c1_se36", "c5_trim_pe150"])
def test_lanes_write_the_side_file_of_one_pipeline(name, tmp_path):
    meta, arr, fasta = G.load(name)
    inputs = _inputs(meta, tmp_path)
    one, two = str(tmp_path / "one.tsv"), str(tmp_path / "two.tsv")
    _run(meta, fasta, inputs, str(tmp_path / "one.sam"), [f"--all-hits={one}"])
    _run(meta, fasta, inputs, str(tmp_path / "two.sam"), [f"--all-hits={two}", "--lanes=2"])
    assert open(one, "rb").read() == open(two, "rb").read() and len(_side(one)) > 0
    assert open(str(tmp_path / "one.sam"), "rb").read() == open(str(tmp_path / "two.sam"), "rb").read()
    assert not os.path.exists(two + ".0") and not os.path.exists(two + ".1")
    files = str(tmp_path / "files.tsv")
    _run(meta, fasta, inputs, str(tmp_path / "files.sam"), [f"--all-hits={files}", "--lanes=2", "--lane-files"])
    parts = [open(f"{files}.{l}").read() for l in range(2)]
    assert all(p.startswith("#name") for p in parts)
    assert parts[0] + parts[1].split("\n", 1)[1] == open(one).read()
