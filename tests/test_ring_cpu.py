"""bsx_ring.h, the ordered hand-offs under the command line's pipeline (Ring: acquire by batch ordinal and stage, the slot's batch ordinal, finish; Gate: compute
slots granted in batch order; LeakChain: a value handed from batch to batch), run alone in the product's thread shape over an int payload
(tests/harness/ring_check.cpp), once under AddressSanitizer + UBSan and once under ThreadSanitizer.  The shapes are the smallest at which the protocol can go
wrong: rings of 6 slots with 1, 2 and 6 middle consumers and of NG + 4 slots with 3, batch counts around the ring size."""
import os
import subprocess

import pytest

from conftest import HOST_SAN_FLAGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSAN_FLAGS = ["-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread"]
SHAPES = [(6, 1), (6, 2), (6, 6), (7, 3)]   # (NS, NG): the command line's ring has max(6, NG + 4) slots


def _counts(ns):
    return [0, 1, ns - 1, ns, ns + 1, 2 * ns + 1, 50]


@pytest.fixture(scope="module", params=["asan", "tsan"])
def harness(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("rh_" + request.param)
    flags = HOST_SAN_FLAGS if request.param == "asan" else TSAN_FLAGS   # (ASan + UBSan: conftest.py)
    if request.param == "tsan":
        # ThreadSanitizer cannot start under some kernels' address-space layouts: the leg is skipped only where an empty program built with the same flags fails
        empty = d / "empty.cpp"
        empty.write_text("int main(){}\n")
        subprocess.run(["g++"] + flags + ["-o", str(d / "empty"), str(empty)], check=True)
        if subprocess.run([str(d / "empty")], capture_output=True, timeout=60).returncode != 0:
            pytest.skip("a ThreadSanitizer program does not start on this machine")
    exe = str(d / "ring_check")
    subprocess.run(["g++"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "harness", "ring_check.cpp")], check=True)
    return exe


def _ok(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout == "ok\n", (args, out.stdout, out.stderr)


def test_every_stage_sees_every_batch_once_in_order_with_its_own_payload(harness):
    for ns, ng in SHAPES:
        for n in _counts(ns):
            _ok(harness, "ring", ns, ng, n, 0)


def test_a_partial_last_batch_released_before_finish_is_delivered(harness):
    """the parse stage's cut at unequal mate files: release(k, 1); k++; finish(k) delivers exactly k batches"""
    for ns, ng in SHAPES:
        for n in _counts(ns):
            _ok(harness, "ring", ns, ng, n, 1)


def test_waiters_behind_the_end_return_false_on_finish(harness):
    for ns, _ in SHAPES:
        for n in (0, 1, ns - 1):
            _ok(harness, "late", ns, n)


def test_gate_holders_and_grant_order(harness):
    for nc in (1, 2):
        for nd in (1, 2):
            _ok(harness, "gate", nc, nd)


def test_leak_chain_applies_the_batches_in_order(harness):
    _ok(harness, "chain")
