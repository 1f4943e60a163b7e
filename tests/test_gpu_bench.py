"""bench.py end to end on the device at a small size: a plain run times the headline only and --dump-outputs
writes what the last timed pass handed back; --full adds the legs beside the headline."""
import json

import numpy as np
import pytest

from test_bench_cpu import _run_bench

pytestmark = pytest.mark.gpu

SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "96", "--committee", "8", "--registry", "4096"]


def _line(p):
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_is_headline_only_and_dumps_outputs(tmp_path):
    d = _line(_run_bench([*SMALL, "--dump-outputs", str(tmp_path / "out")]))
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "FAV/s"
    assert d["ms_per_step"] > 0 and abs(d["value"] - 96 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    for k in ("roofline", "parity", "percall", "cpu_baseline", "host_buffers_fav_s", "gather_hbm_gbs"):
        assert d[k] is None, k
    assert d["kernels_avg_ms"] == {} and not {"registry_load", "c3", "c4", "c5"} & set(d)
    v, ok = np.load(tmp_path / "out" / "verdicts.npy"), np.load(tmp_path / "out" / "batch_ok.npy")
    assert v.dtype == np.float32 and v.shape == (96,) and (v == 1).all()
    assert ok.dtype == np.float32 and ok.tolist() == [1.0]


def test_full_run_adds_the_other_legs():
    d = _line(_run_bench([*SMALL, "--full", "--cpu-seconds", "0.2"]))
    assert d["full"] is True and d["steps"] == 3
    assert d["roofline"]["kernel"] in d["kernels_avg_ms"] and d["host_buffers_fav_s"] > 0
    assert d["percall"]["verify_ms"] > 0 and d["cpu_baseline"]["value"] > 0
