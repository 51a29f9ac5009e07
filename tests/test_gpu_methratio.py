"""bsmap_amd.methratio (Python host + HIP pile-up kernels through the C ABI) against the output of the reference's own
methratio.py (tests/golden/methratio.json.gz, and the hand-made edge set tests/golden/methratio_edges.json.gz: contigs of 1-7
letters, reads across chromosome ends, deep piles, PNEXT cuts): table files byte-identical for every option set, summary line
identical."""
import gzip
import json
import os

import pytest

import golden_util as G
import meth_util as U

pytestmark = pytest.mark.gpu
GOLD = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio.json.gz"), "rt"))
RUNS = [(c, i) for c in sorted(GOLD["cases"]) for i in range(len(GOLD["cases"][c]["runs"]))]
EDGES = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio_edges.json.gz"), "rt"))
EDGE_RUNS = [(c, i) for c in sorted(EDGES["cases"]) for i in range(len(EDGES["cases"][c]["runs"]))]
SETS = {"": GOLD, "edges": EDGES}
ALL_RUNS = [("", c, i) for c, i in RUNS] + [("edges", c, i) for c, i in EDGE_RUNS]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("meth")
    fa = str(d / "g.fa")
    open(fa, "w").write(GOLD["fasta"])
    paths = {}
    for c, case in GOLD["cases"].items():
        for fn, txt in case["files"].items():
            open(str(d / fn), "w").write(txt)
        for fn, b64 in case.get("files_b64", {}).items():
            import base64
            open(str(d / fn), "wb").write(base64.b64decode(b64))
        paths[c] = [str(d / fn) for fn in case["infiles"]]
    return fa, paths, d


@pytest.fixture(scope="module")
def edge_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("meth_edges")
    fa = str(d / "g.fa")
    open(fa, "w", newline="").write(EDGES["fasta"])  # (one record has CRLF line ends, the last line no newline: written as stored)
    paths = {}
    for c, case in EDGES["cases"].items():
        for fn, txt in case["files"].items():
            open(str(d / fn), "w", newline="").write(txt)
        paths[c] = [str(d / fn) for fn in case["infiles"]]
    return fa, paths, d


@pytest.mark.parametrize("gold,case,i", ALL_RUNS,
                         ids=[(g + "-" if g else "") + f"{c}-{'_'.join(SETS[g]['cases'][c]['runs'][i]['options']) or 'default'}" for g, c, i in ALL_RUNS])
def test_methratio_matches_reference_script(gold, case, i, request, capsys):
    from bsmap_amd import methratio
    fa, paths, d = request.getfixturevalue("edge_files" if gold else "files")
    GOLD = SETS[gold]
    run = GOLD["cases"][case]["runs"][i]
    if "same_as" in run:  # the BAM file was converted from that case's SAM file by the vendored samtools: same expected output
        run = [r for r in GOLD["cases"][run["same_as"]]["runs"] if r["options"] == run["options"]][0]
    out = str(d / f"{case}_{i}.txt")
    methratio.main(["-q", "-o", out, "-d", fa] + list(run["options"]) + paths[case])
    assert open(out).read() == run["table"]
    stdout = capsys.readouterr().out
    if not run["crashed"]:
        assert stdout == run["stdout"]


def test_methratio_low_level_calls_agree_with_the_file_path(files):
    """bsx_meth_add with explicit arrays in many small batches (duplicate removal is defined by input order across calls)
    gives the same rows as the file-level call"""
    import numpy as np
    from bsmap_amd import methratio
    fa, paths, d = files
    out = str(d / "file.txt")
    methratio.run(fa, paths["pe"], out, rm_dup=True, meth0=True)
    ref = methratio.load_reference(fa, [])
    names = list(ref)
    st = {"++": 0, "-+": 1, "+-": 2, "--": 3}
    rows = []
    for p_ in paths["pe"]:
        for line in open(p_):
            col = line.split("\t")
            if col[3][:2] in ("NM", "QC"):
                continue
            rows.append((names.index(col[4]), int(col[5]) - 1, st[col[6]], int(col[7]), col[1]))
    with methratio.Meth.from_lengths([len(ref[n]) for n in names], rm_dup=True) as m:
        for i, n in enumerate(names):
            m.set_reference(i, ref[n])
        for b0 in range(0, len(rows), 53):
            part = rows[b0:b0 + 53]
            off = np.cumsum([0] + [len(r[4]) for r in part]).astype(np.uint64)
            seq = np.frombuffer(("".join(r[4] for r in part)).encode() + b"\0", np.uint8)
            m.add_arrays(len(part), np.array([r[0] for r in part], np.uint32), np.array([r[1] for r in part], np.int64), np.array([r[2] for r in part], np.uint8),
                         np.array([r[3] for r in part], np.int32), np.full(len(part), -1, np.int64), seq, off, 2)
        got = [(names[c], pos + 1, dep, met) for c, pos, dep, met in U.table_rows(m, len(names))[0]]
    exp = [(f[0], int(f[1]), int(f[5]), int(f[6])) for f in (l.split("\t") for l in open(out).read().split("\n")[1:] if l)]
    assert sorted(got) == sorted(exp) and len(got) > 1000


@pytest.mark.parametrize("window", ["1", "70000", "1000000"])
def test_methratio_bam_is_streamed_in_bounded_windows(window, files, capsys, monkeypatch):
    """the BAM path inflates a bounded window of BGZF blocks at a time (a whole-genome BAM does not fit host memory): with
    windows of one block, a few blocks, everything — header and records straddling the window edges — the table stays the
    reference's (duplicate removal across windows keeps the file order)"""
    from bsmap_amd import methratio
    fa, paths, d = files
    import bam_util
    case = [c for c in sorted(GOLD["cases"]) if any(p.endswith(".bam") for p in paths[c])][0]
    # the same file in BGZF blocks of 997 bytes: every window edge then cuts through the header or a record
    small = []
    for p_ in paths[case]:
        data, _ = bam_util.read_bgzf(p_)
        q = str(d / ("small_" + os.path.basename(p_)))
        with open(q, "wb") as f:
            for i in range(0, len(data), 997):
                f.write(bam_util._bgzf_block(data[i:i + 997]))
            f.write(bam_util._bgzf_block(b""))
        small.append(q)
    monkeypatch.setenv("BSX_BAM_WINDOW", window)
    for i, run in enumerate(GOLD["cases"][case]["runs"][:6]):
        exp = run
        if "same_as" in run:
            exp = [r for r in GOLD["cases"][run["same_as"]]["runs"] if r["options"] == run["options"]][0]
        out = str(d / f"win_{window}_{i}.txt")
        methratio.main(["-q", "-o", out, "-d", fa] + list(run["options"]) + small)
        assert open(out).read() == exp["table"]
        capsys.readouterr()


def sam_to_bam(sam_text, path, block, rng):
    """the SAM file of the edge set as a BAM file (tests/bam_util.py): same records; in front of ZS:Z a draw of optional fields of
    every type the format has (A c C s S i I f Z H B), which the decoder has to step over"""
    import bam_util
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


@pytest.mark.parametrize("window", ["1", "70000", None])
def test_methratio_edge_pairs_as_bam(window, edge_files, capsys, monkeypatch):
    """the SAM case of the edge set, written as BAM by the test (997-byte BGZF blocks: every window edge cuts the header or a
    record; optional fields of all eleven types in front of ZS:Z), gives the SAM run's table and summary for every option set"""
    import random
    from bsmap_amd import methratio
    fa, paths, d = edge_files
    case = EDGES["cases"]["pairs"]
    bam = str(d / "pairs_twin.bam")
    sam_to_bam(case["files"]["pairs.sam"], bam, 997, random.Random(11))
    if window is None:
        monkeypatch.delenv("BSX_BAM_WINDOW", raising=False)
    else:
        monkeypatch.setenv("BSX_BAM_WINDOW", window)
    for i, run in enumerate(case["runs"]):
        out = str(d / f"twin_{window}_{i}.txt")
        methratio.main(["-q", "-o", out, "-d", fa] + list(run["options"]) + [bam])
        assert open(out).read() == run["table"], run["options"]
        assert capsys.readouterr().out == run["stdout"], run["options"]
