"""The launch plan of every form of a FastAggregateVerify batch, pinned: a host-side slip can leave every verdict
right -- a stage enqueued twice, an idempotent stage skipped, a fold level dropped on a one-level plan -- so each
scenario of tests/launch_plan_scenarios.py is compared with tests/golden/fav_launch_plan.json, recorded
(tools/record_launch_plan.py) from the library as it was before the C ABI was split into csrc/bls_capi_*.hip:
the profiler's launch counts per name (never its times), bls_last_batch_work, after a failing batch
bls_last_fallback_stats, for bits batches bls_last_gather_work.  Every verdict is also checked against the
construction (each signature valid unless the scenario replaces it), as tests/test_gpu_gather.py does."""
import json
import os

import pytest

import launch_plan_scenarios as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "fav_launch_plan.json")) as _fh:
    GOLDEN = json.load(_fh)
SCENARIOS = S.scenarios()


@pytest.fixture(scope="module")
def lib():
    from bls_mi355x import _native, batch

    ctx = _native.context()
    S.load_registry(batch, ctx)
    return batch, ctx


def test_fixture_covers_the_scenarios():
    assert sorted(GOLDEN) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_launch_plan(lib, name):
    batch, ctx = lib
    rec, out, expect = SCENARIOS[name](batch, ctx)
    print(name, json.dumps(rec, sort_keys=True))
    assert list(out) == list(expect), [i for i, (a, b) in enumerate(zip(out, expect)) if a != b]
    assert name.endswith("_valid") == bool(expect.all())
    if "gather_work" in rec:  # mode auto took both forms
        assert 0 < rec["gather_work"][1] < S.SMALL_B
    # (threshold_4096_bad: four pairs share each f there, so its verdicts stand only if the bisection recomputes
    # the per-item f)
    assert rec == GOLDEN[name]
