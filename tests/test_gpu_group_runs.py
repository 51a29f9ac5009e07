"""k_task_groups forms the groups of k_hscan_same over whole runs of a window inside a tile of the scan order (1 024 slots; BSX_GROUP_TILE), not inside 64-slot
segments: the tile is sorted by window, offset class (sub_h & 31), offset and task id, and every run is cut into near-equal groups (bsx_groups.h).  Needs an MI355X.

The world and the helpers are those of tests/test_gpu_group_cap.py (the 421-copy genome, heavy threshold 48, classes of distinct reads unit[a : a + L] that meet
in one window in the first pass, every batch under BSX_SAME_R unset and =16 with the work counters off and on, records against the oracle's, counters 0-3 with the
oracle's when counted, result bytes equal across the four routes).  What is new here is the order in which the reads arrive: the classes of a batch are imported
INTERLEAVED, and with BSX_SPREAD=0 all tasks of the window go to one bin in the order of arrival, so that every 64-slot segment of the scan order holds pieces of
every class — the shape that the segments of round 9 cut into small groups.
  64 + 64, a = 0 and 16 (offsets not congruent mod 32: two sets that no group can share), strictly interleaved: the whole sets are two groups of 64;
  65 + 65: the cut 33 + 32 lies inside a set;
  70 + 3: a set cut 35 + 35 beside a small one;
  30 + 30 + 30 at a = 0, 32, 64 (congruent: one frame holds all 90, cut 45 + 45 across the classes) interleaved with 40 at a = 16 (L = 132, -v 6);
  one offset, as many distinct reads as the construction gives (497), under BSX_GROUP_TILE=64, the smallest tile: the set crosses seven tile borders;
each of the first four plain, with members that carry v + 1 differences (no hit, every list walked) and with members that carry an N in the last word (three
operations per word); those members are the reads at rows 0, 31, 32, 63 and 64 of the interleaved batch.  Where a read's row lies in its group follows the sort,
not the batch: what is asked is that every read is the oracle's record wherever it lies.

That the sets are taken whole is read from the kernel's own statistics (BSX_SIGHIST=1): for 64 + 64 interleaved under BSX_SPREAD=0 the mean group is above 48
under the default cap (the whole sets give 64; 64-slot segments that hold 32 + 32 give 32) and at most 16 under BSX_SAME_R=16."""
import pytest

import test_gpu_group_cap as GC
from test_gpu_group_cap import world  # noqa: F401  (the module's fixture: genome, references, heavy threshold)

pytestmark = pytest.mark.gpu

ROWS = (0, 31, 32, 63, 64)


def interleave(sizes):
    """(class, index in class) by batch row: the classes dealt evenly over the batch — strictly alternating where they are equal"""
    rows = sorted(((i + 0.5) / n, c, i) for c, n in enumerate(sizes) for i in range(n))
    return [(c, i) for _, c, i in rows]


def make_batch(unit, L, v, classes, kind):
    """classes: (a, n) each; the reads interleaved, those at ROWS of the batch of the given kind ('plain': none)"""
    rows = interleave([n for _, n in classes])
    special = [set() for _ in classes]
    if kind != "plain":
        for r in ROWS:
            if r < len(rows):
                special[rows[r][0]].add(rows[r][1])
    by_class = [GC._class(unit, L, a, n, v, tuple(sorted(special[c])), kind) for c, (a, n) in enumerate(classes)]
    reads = [by_class[c][i] for c, i in rows]
    assert len({r["seq"] for r in reads}) == len(reads)
    if kind != "plain":
        want = "_over" if kind == "over" else "_N"
        assert all(want in reads[r]["name"] for r in ROWS if r < len(reads))
    return reads


@pytest.mark.parametrize("kind", ["plain", "over", "N"])
@pytest.mark.parametrize("sizes", [(64, 64), (65, 65), (70, 3)])
def test_two_sets_interleaved_in_one_bin(sizes, kind, world, oracle, monkeypatch):
    monkeypatch.setenv("BSX_SPREAD", "0")
    reads = make_batch(world["unit"], 144, 2, list(zip((0, 16), sizes)), kind)
    exp = GC._run(world, oracle, GC.KW2, reads, monkeypatch, "interleaved %s, %s" % (sizes, kind), 32)
    GC._check_picks(reads, exp)


@pytest.mark.parametrize("kind", ["plain", "over", "N"])
def test_three_congruent_classes_and_a_fourth_set(kind, world, oracle, monkeypatch):
    monkeypatch.setenv("BSX_SPREAD", "0")
    reads = make_batch(world["unit"], 132, 6, [(0, 30), (32, 30), (64, 30), (16, 40)], kind)
    exp = GC._run(world, oracle, GC.KW6, reads, monkeypatch, "30 + 30 + 30 and 40, %s" % kind, 64)
    GC._check_picks(reads, exp)


def test_a_set_that_crosses_tile_borders(world, oracle, monkeypatch):
    unit = world["unit"]
    n = sum(1 for _ in GC._drops(unit, 144, 0))
    assert 64 * 4 < n < 1100, n   # (fewer distinct reads than a tile of 1 024: the smallest tile instead)
    monkeypatch.setenv("BSX_GROUP_TILE", "64")
    reads = make_batch(unit, 144, 2, [(0, n)], "plain")
    exp = GC._run(world, oracle, GC.KW2, reads, monkeypatch, "%d reads of one offset, tiles of 64" % n, 32)
    GC._check_picks(reads, exp)


def test_whole_sets_form_the_groups(world, oracle, monkeypatch, capfd):
    reads = make_batch(world["unit"], 144, 2, [(0, 64), (16, 64)], "plain")
    monkeypatch.setenv("BSX_SPREAD", "0")
    monkeypatch.setenv("BSX_SIGHIST", "1")
    monkeypatch.delenv("BSX_SAME_R", raising=False)
    mg = GC._mean_group(world, reads, capfd)
    monkeypatch.setenv("BSX_SAME_R", "16")
    mg16 = GC._mean_group(world, reads, capfd)
    print("mean group, 64 + 64 interleaved in one bin: default cap %.2f, BSX_SAME_R=16 %.2f" % (mg, mg16))
    assert mg > 48.0, mg
    assert mg16 <= 16.0, mg16
