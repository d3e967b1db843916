"""Host-side behaviour of bench.py that needs no GPU: the launcher of `--gpus N` must not outlive a dead
rank, and the RCCL summary parser must take whatever the log holds."""
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_a_dead_rank_ends_the_run_with_a_reason():
    """No GPU here: every rank dies at `torch.cuda.set_device`.  The parent reports the first failure on one
    line, stops the others and exits non-zero — it does not wait for a rendezvous that cannot happen."""
    t0 = time.time()
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--no-cpu-baseline", "--no-api", "--no-pmc"], capture_output=True, text=True, timeout=300,
                       env={**__import__("os").environ, "S3GRL_BENCH_BACKEND": "gloo", "S3GRL_BENCH_RENDEZVOUS_S": "20",
                            "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    assert r.returncode != 0
    lines = [ln for ln in r.stderr.splitlines() if "bench.py --gpus 2 FAILED:" in ln]
    assert len(lines) == 1 and "rank" in lines[0], r.stderr[-2000:]
    assert r.stdout.strip() == ""                      # no JSON line from a failed run
    assert time.time() - t0 < 240


def test_rccl_summary_never_raises(tmp_path):
    sys.path.insert(0, str(REPO))
    import bench

    log = tmp_path / "rccl.log"
    log.write_text("h:1:1 [0] NCCL INFO NCCL version 2.22.3 / RCCL\n"
                   "h:1:1 [0] NCCL INFO Channel 00/16 :    0   1\n"
                   "h:1:1 [0] NCCL INFO Channel 00 : 0[0] -> 1[1] via P2P/IPC\n"
                   "h:1:1 [0] NCCL INFO Connected all rings\n"
                   "garbage line without the marker\n")
    s = bench.rccl_summary(log)
    assert s["channels"] == 16 and s["connections_via"] == {"P2P/IPC": 1} and "rings_connected" in s
    assert "error" in bench.rccl_summary(tmp_path / "missing.log")
    (tmp_path / "empty.log").write_text("")
    assert bench.rccl_summary(tmp_path / "empty.log")["info_lines"] == 0


def test_steps_must_be_at_least_one():
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


def test_counter_passes_belong_to_full_runs():
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), "--collect-pmc"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--collect-pmc needs --full" in r.stderr


def test_dump_outputs_fits_its_budget_and_repeats(tmp_path, monkeypatch):
    """--dump-outputs on host tensors: float32 / float64 files only, at most DUMP_BYTES in all, the same sample
    from run to run, and what it writes is what the rows hold."""
    import numpy as np
    import torch

    sys.path.insert(0, str(REPO))
    import bench

    monkeypatch.setattr(bench, "DUMP_BYTES", 1_000_000)
    g = torch.Generator().manual_seed(0)
    rows = torch.randn((3000, 4, 65), generator=g)                       # 3.1 MB: sampled
    row_ptr = torch.arange(0, 3001, 2, dtype=torch.int64)
    for d in ("a", "b"):
        bench.dump_outputs(tmp_path / d, rows, row_ptr)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["row_ptr.npy", "rows_colsum.npy", "rows_sample.npy", "rows_sample_index.npy"]
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= bench.DUMP_BYTES
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    idx = np.load(tmp_path / "a" / "rows_sample_index.npy").astype(np.int64)
    assert 0 < len(idx) < 3000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rows_sample.npy"), rows.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "row_ptr.npy"), row_ptr.numpy().astype(np.float64))
    np.testing.assert_allclose(np.load(tmp_path / "a" / "rows_colsum.npy"),
                               rows.numpy().astype(np.float64).sum(axis=0), rtol=1e-12, atol=1e-9)

    small = rows[:100].double()                                           # fits: every row, float64 kept
    bench.dump_outputs(tmp_path / "c", small, row_ptr[:51])
    assert np.array_equal(np.load(tmp_path / "c" / "rows_sample_index.npy"), np.arange(100.0))
    assert np.array_equal(np.load(tmp_path / "c" / "rows_sample.npy"), small.numpy())
