"""k_hscan_same's groups on the reverse-strand copy, for pairs and at the ends of the reference: the directed reads of tests/test_oracle_group_strands.py — where
the constructions are described and checked against the oracle on the CPU — through the device.  Needs an MI355X.

Every batch is compared with the oracle unit by unit as tests/test_gpu_boundaries.py does (all class counts, every hit list of both orientations, the pick; pairs:
paired, n_pairs, every pair list, the pick, unpaired_out and the same per mate), under the routes BSX_SAME_D / BSX_SAME_R unset, BSX_SAME_D=0 and BSX_SAME_R=16, each
with the work counters off (the exiting evaluation for reads of 129-160 letters) and on; counters 0-3 are the oracle's when counted, and the result bytes of all routes
of a batch are equal.  The construction's own claims (which copies are hits, where the oracle reports a reverse hit, which reads meet in one window in the first pass,
which members stick out of a chromosome) are asserted from the oracle's records before the device is asked.  Counter 15 (candidates evaluated in groups of two reads
and more) must be above 0 wherever two reads meet, and 0 under BSX_SAME_D=0 in the batches that hold one read per strand, length and offset: a strand-0 and a strand-1
task of equal n, length and offset stand next to each other there and must stay groups of one.

What the module is for: hs_group reporting strand 0 for every survivor, and the frame's move leaving the positions where they were, fail it; a group's
survivors on the reverse copy, of an offset class behind the first, and at a chromosome's first and last letters are compared nowhere else."""
import pytest

import bsmap_amd as B
import test_gpu_boundaries as GB
import test_oracle_group_strands as S

pytestmark = pytest.mark.gpu

ROUTES = ((None, None), ("BSX_SAME_D", "0"), ("BSX_SAME_R", "16"))
OFFSET_BATCHES = ["offsets L%d -v %d %s" % (L, v, k) for v, L in ((2, 144), (6, 132)) for k in ("within", "over", "N")]
CAP_BATCHES = ["cap %s %s" % (sz, k) for sz in ((65,), (40, 30)) for k in ("plain", "over", "N")]
EDGE_BATCHES = ["edges L%d -v %d %s" % (L, v, k) for v, L in ((6, 132), (2, 144)) for k in ("plain", "over", "N")]


class _World:
    """a genome with its reference on the device and in the oracle, per set of options; the heavy threshold is 48 while the module runs"""

    def __init__(self, oracle, w):
        self.oracle, self.w, self.refs = oracle, w, {}

    def ref(self, kw):
        k = tuple(sorted(kw.items()))
        if k not in self.refs:
            self.refs[k] = (self.oracle.OracleRef(self.oracle.make_params(**kw), fasta_text=self.w["fasta"]),
                            B.RefSeq(B.make_params(**kw)).Run_ConvertBinseq(fasta_text=self.w["fasta"]).CreateIndex())
        return self.refs[k]

    def close(self):
        for oref, gref in self.refs.values():
            gref.close()
            oref.free()


@pytest.fixture(scope="module", autouse=True)
def heavy_threshold():
    B.lib().bsx_set_heavy_threshold(48)
    yield
    B.lib().bsx_set_heavy_threshold(0)


@pytest.fixture(scope="module")
def strands(oracle):
    w = _World(oracle, S.make_strand_world())
    S.check_buckets_strands(w.ref(S.KW[2])[0], w.w)
    yield w
    w.close()


@pytest.fixture(scope="module")
def edges(oracle):
    w = _World(oracle, S.make_edge_world())
    S.check_edge_buckets(w.ref(S.KW[2])[0], w.w)
    yield w
    w.close()


def _run(world, kind, kw, reads, monkeypatch, name, check=None, routes=ROUTES, groups=True, alone_without_d=False):
    """one batch through the routes, against the oracle.  check(exp): the construction's claims, from the oracle's records, before the device is asked; groups:
    counter 15 must be above 0 (on every route but BSX_SAME_D=0 where alone_without_d, which must then show 0)"""
    oref, gref = world.ref(kw)
    exp, cnt = GB._expected(world.oracle, oref, kind, kw, reads, 0)
    if check:
        check(exp)
    got = {}
    for var, val in routes:
        for v in ("BSX_SAME_D", "BSX_SAME_R"):
            monkeypatch.delenv(v, raising=False)
        if var:
            monkeypatch.setenv(var, val)
        for counters in (False, True):
            route = "%s, %s=%s, counters %s" % (name, var, val, counters)
            if kind == "pe":
                bt = B.PairAlign(gref, len(reads), debug=True)    # (the switches are read when the batch is created)
            else:
                bt = B.SingleAlign(gref, len(reads), debug=True)
            try:
                bt.set_work_counters(counters)
                if kind == "pe":
                    bt.ImportBatchReads([r["seq1"] for r in reads], [r["seq2"] for r in reads], [r["qual1"] for r in reads], [r["qual2"] for r in reads])
                else:
                    bt.ImportBatchReads([r["seq"] for r in reads], [r["qual"] for r in reads])
                bt.Do_Batch()
                res = bt.results()
                GB._compare(kind, kw, reads, exp, bt, res, route)
                c = bt.counters()
                print("%s: heavy units %d, counter 15 %d, counters 0-3 %s oracle %s" % (route, bt.heavy_units(), int(c[15]), [int(x) for x in c[:4]], cnt))
                assert bt.heavy_units() > 0, route
                if alone_without_d and var == "BSX_SAME_D":
                    assert int(c[15]) == 0, (route, int(c[15]))    # no two tasks of equal window, strand, length and offset
                elif groups:
                    assert int(c[15]) > 0, route                   # hs_group ran
                if counters:
                    assert [int(x) for x in c[:4]] == cnt, (route, [int(x) for x in c[:4]], cnt)
                got[(var, counters)] = tuple(a.tobytes() for a in res)
            finally:
                bt.close()
    assert len(set(got.values())) == 1, [k for k in got if got[k] != got[(None, False)]]
    return exp


@pytest.mark.parametrize("L", S.WORD_LENGTHS)
@pytest.mark.parametrize("v", [2, 6])
def test_word_cases_on_both_strands(v, L, strands, monkeypatch):
    reads = S.word_reads(strands.w, v, L)
    _run(strands, "se", S.KW[v], reads, monkeypatch, "words -v %d L %d" % (v, L), check=lambda exp: S.check_word_records(strands.w, reads, exp, v))


def test_word_cases_with_both_orientations(strands, monkeypatch):
    reads = S.n1_reads(strands.w)
    _run(strands, "se", S.KW_N1, reads, monkeypatch, "-n 1", check=lambda exp: S.check_n1_records(strands.w, reads, exp))


def _batch(batches, name):
    return [b for b in batches if b["name"] == name][0]


@pytest.mark.parametrize("name", OFFSET_BATCHES)
def test_offset_classes_on_both_strands(name, strands, monkeypatch):
    b = _batch(S.offset_batches(strands.w), name)

    def check(exp):
        S.check_meet(strands.w, b, exp)
        S.check_strand_neighbours(b)
        S.check_picks(strands.w, b, exp)
    _run(strands, "se", S.KW[b["v"]], b["reads"], monkeypatch, name, check=check, alone_without_d=True)


@pytest.mark.parametrize("name", CAP_BATCHES)
def test_group_cap_on_both_strands(name, strands, monkeypatch):
    b = _batch(S.cap_batches(strands.w), name)

    def check(exp):
        S.check_meet(strands.w, b, exp)
        S.check_picks(strands.w, b, exp)
    _run(strands, "se", S.KW[2], b["reads"], monkeypatch, name, check=check)


def test_both_strands_in_one_list(oracle, monkeypatch):
    """chrM the reverse complement of chrR itself: every list is 421 forward and 421 reverse entries in one task that spans two sub-ranges — a group of one, evaluated by the
    one-task path across the change of strand copy.  Counter 15 is printed, not asked for (see the CPU module's text)"""
    w = _World(oracle, S.make_strand_world(both=True))
    try:
        S.check_buckets_strands(w.ref(S.KW[2])[0], w.w)
        reads = [r for r in S.word_reads(w.w, 2, 144) if r["strand"] == 0]
        _run(w, "se", S.KW[2], reads, monkeypatch, "both strands in one list", check=lambda exp: S.check_word_records(w.w, reads, exp, 2), groups=False)
    finally:
        w.close()


@pytest.mark.parametrize("L", S.PE_LENGTHS)
def test_pairs_on_both_strands(L, strands, monkeypatch):
    pairs = S.pair_cases(strands.w, L)
    _run(strands, "pe", S.KW_PE, pairs, monkeypatch, "pairs L %d" % L, check=lambda exp: S.check_pair_records(strands.w, pairs, exp), routes=(ROUTES[0], ROUTES[2]))


@pytest.mark.parametrize("name", EDGE_BATCHES)
def test_groups_at_the_edges_of_the_reference(name, edges, monkeypatch):
    b = _batch(S.edge_batches(edges.w), name)

    def check(exp):
        if b["kind"] == "plain" and b["meet"] == 64:
            S.check_pack(edges.ref(S.KW[6])[0], edges.w, [r for r in b["reads"] if r.get("pack")])
        S.check_meet(edges.w, b, exp)
        S.check_strand_neighbours(b)
        S.check_edges(edges.w, b, exp)
    _run(edges, "se", S.KW[b["v"]], b["reads"], monkeypatch, name, check=check)
