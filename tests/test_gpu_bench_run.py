"""GPU: a plain bench.py run end to end at a small size -- the last stdout line carries the contract keys for the steps asked
for, no side row runs without --full, and --dump-outputs writes C of the last timed step, the product of the run's seeded operands."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, ATOL = 2 ** -10, 2e-3  # one fp16 ulp of the fp32 truth (tests/test_gpu_hgemm.py)


def test_plain_run_prints_the_line_and_dumps_c(built, dev, tmp_path):
    M = 1024
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--mnk", str(M),
           "--prewarm", "0", "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.rstrip("\n").split("\n")[-1])
    assert line["metric"] == "HGEMM fp16 TFLOPS at M=N=K=%d" % M and line["unit"] == "TFLOPS" and line["dtype"] == "f16"
    assert line["higher_is_better"] is True and line["steps"] == 5 and line["ms_per_step"] > 0 and line["value"] > 0
    assert "cpu_baseline" not in line and "rocblas_tflops" not in line.get("digest", {})  # side rows belong to --full
    c = np.load(tmp_path / "out" / "c.npy")
    assert c.dtype == np.float32 and c.shape == (M, M)
    torch.manual_seed(1234)  # bench.py's operands of rank 0
    a = torch.randn(M, M, dtype=torch.half, device=dev)
    b = torch.randn(M, M, dtype=torch.half, device=dev)
    truth = a.cpu().float() @ b.cpu().float()
    err = (torch.from_numpy(c) - truth).abs()
    bad = (err > ATOL + RTOL * truth.abs()).sum().item()
    assert bad == 0, "mismatches=%d max_err=%g" % (bad, err.max().item())
