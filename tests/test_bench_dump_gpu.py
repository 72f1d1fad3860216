"""GPU: a plain `bench.py` run times exactly --steps steps, reports `ms_per_step`, leaves the `--full` measurements out,
and `--dump-outputs` writes the last timed step's outputs as finite float32 arrays within the size limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_dumps_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT",
                                                            "OTGAN_DIST_BACKEND", "OTGAN_FORCE_COLLECTIVES")}
    d = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch_per_gpu", "64", "--nr_sinkhorn_iter", "20", "--dump-outputs", str(d)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["higher_is_better"] is True and line["unit"] == "images/sec"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(64 * 1e3 / line["ms_per_step"], rel=1e-2)
    assert not {"roofline", "kernel_classes", "secondary", "cpu_baseline"} & set(line)
    assert "rank_times" not in line["config"]
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert set(out) == {"distance", "entropy", "generator_weights", "critic_weights", "generator_ema_weights"}
    assert sum(v.nbytes for v in out.values()) <= 64 << 20
    for k, v in out.items():
        assert v.dtype == np.float32 and v.size > 0 and np.isfinite(v).all(), k
    assert float(out["distance"][0]) == pytest.approx(line["config"]["last_distance"], rel=1e-6)
