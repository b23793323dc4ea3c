"""bench.py's plain run on the GPU: it times exactly --steps steps, prints the headline fields and nothing measured beside them,
and --dump-outputs writes what the last timed step returned (float32 / float64 .npy, sampled when large, within 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "2", "--size", "129",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert abs(line["value"] - 2 * 3 / (3 * line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    for key in ("roofline", "cpu_baseline", "bf16", "gmmn", "shard", "ddp_one_rank", "host_batches"):
        assert key not in line, key
    files = sorted(os.listdir(out))
    assert files == ["logits.npy", "loss.npy", "params.npy"], files
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    assert arrays["logits"].shape == (2, 21, 129, 129)              # below the sample size: the whole tensor
    assert arrays["params"].shape == (1 << 20,)                     # 59 M parameters: the seeded sample
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert float(arrays["loss"]) == pytest.approx(line["last_loss"], rel=1e-6)   # the dump is the last timed step's
