"""The methylation-ratio oracle (oracle/methratio_oracle.py) against the output of the reference's own methratio.py on BSP
files written by the real bsmap binary (tests/golden/methratio.json.gz, made by tests/golden/make_golden_methratio.py), and
on the hand-made edge set (tests/golden/methratio_edges.json.gz, make_golden_methratio_edges.py: contigs of 1-7 letters, reads
across chromosome ends, inserts around the read length, deep piles, PNEXT cuts) that the scale tests of the GPU tool lean on."""
import gzip
import json
import os

import pytest

import golden_util as G
from oracle import methratio_oracle as MO

GOLD = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio.json.gz"), "rt"))
# (the BAM case is the paired SAM case in another container: the oracle reads text, the GPU tool decodes the BAM itself)
RUNS = [(c, i) for c in sorted(GOLD["cases"]) if not c.endswith("_bam") for i in range(len(GOLD["cases"][c]["runs"]))]


@pytest.mark.parametrize("case,i", RUNS, ids=[f"{c}-{'_'.join(GOLD['cases'][c]['runs'][i]['options']) or 'default'}" for c, i in RUNS])
def test_oracle_matches_reference_script(case, i):
    c = GOLD["cases"][case]
    run = c["runs"][i]
    table, summary = MO.run(GOLD["fasta"], [(f, c["files"][f]) for f in c["infiles"]], MO.options_from_argv(run["options"]))
    assert table == run["table"]
    if run["crashed"]:
        assert summary is None  # nothing covered: the reference divides by zero in its last print
    else:
        assert summary == run["stdout"]


EDGES = json.load(gzip.open(os.path.join(G.GOLDEN, "methratio_edges.json.gz"), "rt"))
EDGE_RUNS = [(c, i) for c in sorted(EDGES["cases"]) for i in range(len(EDGES["cases"][c]["runs"]))]


@pytest.mark.parametrize("case,i", EDGE_RUNS, ids=[f"{c}-{'_'.join(EDGES['cases'][c]['runs'][i]['options']) or 'default'}" for c, i in EDGE_RUNS])
def test_oracle_matches_reference_script_on_the_edge_set(case, i):
    c = EDGES["cases"][case]
    run = c["runs"][i]
    assert not run["crashed"]  # (the generator refuses to store a crashed run: it would pin nothing)
    table, summary = MO.run(EDGES["fasta"], [(f, c["files"][f]) for f in c["infiles"]], MO.options_from_argv(run["options"]))
    assert table == run["table"]
    assert summary == run["stdout"]
