"""bench.py's command line: a plain run prints the headline line alone, `--full` is the switch
for everything that takes runs of its own, and `--dump-outputs DIR` writes what the last timed
step returned. CPU: the options and the fixed row sample. GPU: one plain run on the smallest
bench graph (flickr-shaped), its line and its dump checked against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

import bench  # noqa: E402  (ROOT is on sys.path: tests/conftest.py)

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps",
                 "warmup", "n_gpus", "config", "data", "topology"}
FULL_ONLY_KEYS = {"roofline", "fwd_ms", "bwd_ms", "topk_ms", "k_sweep", "comparator",
                  "cpu_baseline", "exchange", "fwd_launch_ms", "bwd_launch_ms"}


def test_full_and_dump_outputs_are_off_by_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None
    assert (a.steps, a.warmup) == (7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_rows_fixed_sample_within_the_share():
    assert bench.dump_rows(100, 256, 100 * 256 * 4) is None          # fits: every row
    share = bench.DUMP_BUDGET_BYTES // 2
    n, d = 232_965, 256                                              # the Reddit forward output
    pick = bench.dump_rows(n, d, share)
    assert pick.size * d * 4 <= share < (pick.size + 1) * d * 4
    assert np.all(np.diff(pick) > 0) and 0 <= pick[0] and pick[-1] < n
    assert np.array_equal(pick, bench.dump_rows(n, d, share))        # the same rows every time
    assert 2 * share <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_headline_line_and_dump(gpu, tmp_path):
    from maxk_kernels import graphs
    from oracle import oracle

    steps, warmup, d, k = 3, 1, 256, 16
    out_dir = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dataset", "flickr", "--graph", "synthetic",
                        "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    rec = json.loads(lines[0])
    assert HEADLINE_KEYS <= set(rec), sorted(rec)
    assert not FULL_ONLY_KEYS & set(rec), sorted(rec)
    assert rec["full"] is False
    assert (rec["steps"], rec["warmup"], rec["n_gpus"]) == (steps, warmup, 1)
    assert rec["metric"] == bench.METRIC and rec["unit"] == "edges/s"
    assert rec["higher_is_better"] is True and rec["dtype"] == "f32"
    e = rec["config"]["num_edges"]
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(2.0 * e / (rec["ms_per_step"] * 1e-3), rel=1e-9)

    assert sorted(os.listdir(out_dir)) == ["grad_sp.npy", "out.npy"]
    out = np.load(out_dir / "out.npy")
    grad_sp = np.load(out_dir / "grad_sp.npy")
    assert out.dtype == np.float32 and grad_sp.dtype == np.float32
    assert out.nbytes + grad_sp.nbytes <= 64 * 10**6

    # the bench's inputs, drawn on the device as the bench draws them
    ptr, idx = graphs.bench_csr("flickr", device=gpu)
    n = ptr.numel() - 1
    assert int(ptr[-1]) == e
    val = graphs.sage_mean_values(ptr)
    h = graphs.features(n, d, seed=97, device=gpu).cpu().numpy()
    g = graphs.features(n, d, seed=98, device=gpu).cpu().numpy()
    ptr, idx, val = ptr.cpu().numpy(), idx.cpu().numpy(), val.cpu().numpy()
    od, oi = oracle.maxk(h, k)
    share = bench.DUMP_BUDGET_BYTES // 2
    for got, cols, (ref, mag) in (
            (out, d, oracle.spgemm_forward(ptr, idx, val, od, oi, d, with_mag=True)),
            (grad_sp, k, oracle.sspmm_backward(ptr, idx, val, g, oi, with_mag=True))):
        pick = bench.dump_rows(n, cols, share)
        if pick is not None:
            ref, mag = ref[pick], mag[pick]
        assert got.shape == ref.shape
        ok, worst = oracle.close_enough(got, ref, mag)
        assert ok, worst
