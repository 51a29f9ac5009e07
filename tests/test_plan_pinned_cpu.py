"""bsx_batch_plan_bytes, pinned: the three numbers (per-unit arrays, per-wave slabs, heavy-pipeline pools at their starting size) for a fixed list of
inputs, as literals.  The plan is what bench.py and tests/test_bench_memory_cpu.py trust to keep a run inside the device, and the allocator walks the same
lists the plan sums — a change of either shows here.  The literals were recorded from the commit BEFORE the plan and the allocator were made one (a build
of that commit, the same inputs), never from the code under test."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bsmap_amd as B  # noqa: E402

spec = importlib.util.spec_from_file_location("bench_mod_pinned", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)

ENTRIES = {"pe": 1_476_000_000, "se": 1_476_000_000, "trim": 1_476_000_000, "rrbs": 56_000_000}   # (as tests/test_bench_memory_cpu.py; n_cu 256, 5 blocks per CU: plan_bytes' defaults)

# (mode, units, starting pools or None = the library's, environment)
CASES = [(m, u, None, {}) for m in ("se", "pe", "rrbs", "trim") for u in (1 << 20, 1 << 22)]
CASES += [(m,) + bench.mode_defaults(m)[::2] + ({},) for m in ("trim", "rrbs")]   # bench.py's own step size and pools where it sets them
CASES += [("pe", 4096, None, {}), ("pe", 1 << 20, (2048, 8192), {}), ("pe", 1 << 20, None, {"BSX_HEAVY_GROUPS": "2"}), ("pe", 1 << 20, None, {"BSX_BIN_LOG2": "16"}),
          ("rrbs", 1 << 20, None, {"BSX_HEAVY_GROUPS": "2"})]

EXPECTED = {
    "se-1048576": (436208144, 1462763520, 37207978632),
    "se-4194304": (1744830992, 1462763520, 45877605000),
    "pe-1048576": (964690968, 5138022400, 36771673896),
    "pe-4194304": (3858760728, 5138022400, 59703150504),
    "rrbs-1048576": (436208144, 21856256000, 61423815176),
    "rrbs-4194304": (1744830992, 21856256000, 61423815176),
    "trim-1048576": (964690968, 5138022400, 36771673896),
    "trim-4194304": (3858760728, 5138022400, 59703150504),
    "trim-3145728-31457,2500000": (2894070808, 5138022400, 52445554408),
    "rrbs-4194304-160000,1900000": (1744830992, 21856256000, 54725481736),
    "pe-4096": (3769368, 4110417920, 6314917640),
    "pe-1048576-2048,8192": (964690968, 5138022400, 2147254024),
    "pe-1048576-BSX_HEAVY_GROUPS=2": (964690968, 5138022400, 36783207984),
    "pe-1048576-BSX_BIN_LOG2=16": (964690968, 5138022400, 36760500264),
    "rrbs-1048576-BSX_HEAVY_GROUPS=2": (436208144, 21856256000, 61430816912),
}


def case_id(c):
    mode, units, limits, env = c
    return "-".join([mode, str(units)] + (["%d,%d" % limits] if limits else []) + ["%s=%s" % kv for kv in sorted(env.items())])


def plan_of(c):
    mode, units, limits, env = c
    M = bench.MODES[mode]
    L = B.lib()
    old = {k: os.environ.get(k) for k in env}
    try:
        os.environ.update(env)
        assert L.bsx_set_heavy_limits(*(limits or (0, 0))) == 0
        d = B.plan_bytes(B.make_params(**M["kw"]), units, M["pe"], ENTRIES[mode])
    finally:
        L.bsx_set_heavy_limits(0, 0)
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return (d["per_unit"], d["scratch"], d["pools"])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_plan_bytes_are_the_recorded_ones(case):
    assert plan_of(case) == EXPECTED[case_id(case)]


if __name__ == "__main__":   # prints the table above (run against a build of the commit whose plan is the reference)
    for c in CASES:
        print('    "%s": %r,' % (case_id(c), plan_of(c)))
