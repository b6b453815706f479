"""The final stdout line of bench.py must stay parsable by the driver (8 KB stdout tail, LAST line parsed).

Round 4 lost its driver-timed headline because the one JSON line had grown to 23 KB (BENCH_r04.json: parsed null).
`bench.headline_line` builds the compact line from the full result; this test holds it under 4 KB on the largest
result the repository has produced (profiles/r04_bench_20steps.json, 23 KB) and on a worst case where every free-text
field is inflated and every optional key is present.
"""
import io
import json
import os
import sys
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (imports torch; no GPU needed to build the line)

REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")
ROOFLINE_KEYS = ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "avg_launch_ms",
                 "algorithmic_flops_per_launch", "algorithmic_bytes_per_launch")
CPU_KEYS = ("value", "unit", "cores", "kind", "sample")


def _canned():
    return json.load(open(os.path.join(ROOT, "profiles", "r04_bench_20steps.json")))


def _inflate(node, n=400):
    """every string -> n characters, every list of rows doubled: a result far larger than any real one"""
    if isinstance(node, dict):
        return {k: _inflate(v, n) for k, v in node.items()}
    if isinstance(node, list):
        return [_inflate(v, n) for v in node] * 2
    if isinstance(node, str):
        return (node + " ") * (n // (len(node) + 1) + 1)
    return node


def _check(line):
    assert "\n" not in line
    assert len(line.encode()) < bench.MAX_LINE <= 4096
    d = json.loads(line)
    for k in REQUIRED:
        assert k in d, k
    assert "workload" in d["config"] and "kernel" in d["config"] and "parallelism" in d["config"]
    for k in ROOFLINE_KEYS:
        assert k in d["roofline"], k
    for k in CPU_KEYS:
        assert k in d["cpu_baseline"], k
    return d


def test_largest_real_result_fits():
    out = _canned()
    assert len(json.dumps(out)) > 20000  # the line that did not parse in round 4
    d = _check(bench.headline_line(out))
    assert d["value"] == out["value"] and d["ms_per_step"] == out["ms_per_step"]
    assert d["roofline"]["frac"] == out["roofline"]["frac"]
    assert d["digest"]["fa2_fwd"]["c4_d64"]["tflops"] == out["roofline_fa2_c4_d64"]["achieved"]
    assert d["digest"]["pct_of_rocblas"] == out["extras"]["pct_of_rocblas"]


def test_inflated_worst_case_fits():
    out = _inflate(_canned())
    out["extras"]["fa2_error"] = "x" * 5000
    out["extras"]["rocblas_error"] = "y" * 5000
    out["pmc"] = {"status": "z" * 3000, "seconds": 9.9}
    for k in ("value", "ms_per_step", "steps", "warmup", "n_gpus"):
        out[k] = _canned()[k]
    _check(bench.headline_line(out))


def test_multi_gpu_result_without_side_rows_fits():
    out = {k: v for k, v in _canned().items() if k not in ("extras", "configs", "cpu_baseline") and not k.startswith("roofline_fa2")}
    line = bench.headline_line(out)
    d = json.loads(line)
    assert len(line) < bench.MAX_LINE and "roofline" in d and "cpu_baseline" not in d  # rank 0 of N>1 has no CPU leg


def test_emit_prints_headline_last_and_rows_are_short(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    buf = io.StringIO()
    with redirect_stdout(buf):
        bench.emit(_canned())
    lines = buf.getvalue().rstrip("\n").split("\n")
    _check(lines[-1])
    assert all(len(x) <= 200 and x.startswith("#") for x in lines[:-1])
    assert len(lines) > 30  # one row per measured kernel / config, as the reference scripts print
    full = json.load(open(tmp_path / "bench_detail.json"))
    assert full["configs"]["bandwidth"] == _canned()["configs"]["bandwidth"]  # nothing is lost: the detail file has every row
    # the driver's 8 KB tail always holds the whole final line
    tail = buf.getvalue()[-8192:]
    assert json.loads(tail.rstrip("\n").split("\n")[-1])["metric"].startswith("HGEMM")


def test_plain_run_takes_no_side_rows_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_rows_are_a_fixed_sample_under_64_mb():
    import torch
    assert torch.equal(bench.dump_rows(1024, 1024), torch.arange(1024))  # small outputs are written whole
    r = bench.dump_rows(4096, 4096)
    assert torch.equal(r, bench.dump_rows(4096, 4096))  # the same rows in every run
    assert r.numel() * 4096 * 4 <= bench.DUMP_ELEMS * 4 <= 64 << 20
    assert r.numel() == len(set(r.tolist())) and bool((r[1:] > r[:-1]).all()) and 0 <= int(r[0]) and int(r[-1]) < 4096


def test_dump_outputs_writes_float32_rows_of_c(tmp_path):
    import numpy as np
    import torch
    c = torch.randn(4096, 2048, generator=torch.Generator().manual_seed(3)).half()
    bench.dump_outputs(str(tmp_path / "out"), c)
    x = np.load(tmp_path / "out" / "c.npy")
    assert x.dtype == np.float32 and x.shape == (2048, 2048)
    assert np.array_equal(x, c[bench.dump_rows(4096, 2048)].float().numpy())
