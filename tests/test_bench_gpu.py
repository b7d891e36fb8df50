"""GPU: bench.py itself on the real kernel, a plain run (no --full) with
--dump-outputs: the line's headline figures, nothing of a full run in it, and
the dumped state bit-exact against the oracle's Step() of the same seeded
fill.  4099 universes: more than one block, no multiple of the 4 universes a
wave takes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path, port):
    n, steps, warmup = 4099, 3, 2
    d = str(tmp_path / "out")
    env = dict(os.environ, LIFEAPI_BENCH_DETAIL=str(tmp_path / "detail.json"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "LIFEAPI_BENCH_BACKEND"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--universes", str(n),
                        "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", d],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["full"] is False and "kernel_backend" not in line
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(n / (line["ms_per_step"] / 1e3), rel=1e-9)
    assert line["unit"] == "universe-gen/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    for key in ("verified", "collect", "cpu_baseline", "value_hbm_only"):
        assert line[key] is None, key
    assert line["roofline"]["hbm_only"] is None and not os.path.exists(env["LIFEAPI_BENCH_DETAIL"])
    assert line["outputs"]["universes_written"] == n
    f = np.load(os.path.join(d, "state_words16.npy"))
    u = np.load(os.path.join(d, "state_universe.npy"))
    assert f.dtype == np.float32 and f.shape == (n, 64, 4) and u.dtype == np.float64
    assert (u == np.arange(n)).all()
    q = f.astype(np.uint64)
    got = q[..., 0] | q[..., 1] << np.uint64(16) | q[..., 2] << np.uint64(32) | q[..., 3] << np.uint64(48)
    # one launch before the W - 1 further warm ones, then the K timed steps
    assert (got == port.step_batch(port.fill(n, seed=2), 1 + (warmup - 1) + steps)).all()
