"""SAGE and GIN (s3grl_amd.mpnn / mpgnn) on the GPU against their torch restatement in the same process, alternated:
  * the warm median epoch time of the Table 2 loop (`mpgnn.train`) for SAGE and GIN on USAir (x = None) and on Cora's
    bag-of-words rows;
  * one SEAL epoch plus the test pass (`harness.train_and_evaluate_seal_mpnn`, epochs = 1) of SAGETwin and GINTwin on
    USAir 2-hop subgraphs, hidden 32;
  * with --thresholds, the test AUC of both sides for seeds 1, 2, 3 on USAir (50 MPGNN epochs; 4 SEAL epochs at lr
    1e-3): the restatement's minima are the floors of tests/test_gpu_mpnn.py.
The restatement replaces the two HIP operators by torch ops on the device: index_add aggregation over the edge list
and a scatter-style mean pool; everything else (loop, negatives, decoder, optimiser) is shared.  Times are wall clock
around device synchronisation, warm-up excluded.  Writes profiles/mpgnn_probe.json.

    python tools/mpgnn_probe.py [--out FILE] [--reps R] [--only-hip] [--thresholds]

Run it under `rocprofv3 --kernel-trace --stats` with `--only-hip` for the two new kernels' share of an epoch.
"""
import argparse
import contextlib
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from s3grl_amd import harness, mpgnn, mpnn  # noqa: E402
from s3grl_amd import workloads as W  # noqa: E402
from s3grl_amd.seal import enclosing_subgraphs  # noqa: E402

DEV = "cuda:0"
WARM = 5


def _torch_aggregate(h, op, mode, self_coef=0.0):
    ei = op.edge_index
    out = torch.zeros_like(h).index_add_(0, ei[1], h[ei[0]])
    if mode == "mean":
        deg = torch.zeros(h.shape[0], device=h.device).index_add_(0, ei[1], torch.ones_like(ei[1], dtype=h.dtype))
        out = out / deg.clamp(min=1)[:, None]
    return out + self_coef * h if self_coef else out


def _torch_segment_mean(x, node_ptr, max_nodes=None):
    counts = node_ptr.diff()
    G = counts.numel()
    graph = torch.repeat_interleave(torch.arange(G, device=x.device), counts, output_size=x.shape[0])
    out = torch.zeros((G, x.shape[1]), dtype=x.dtype, device=x.device).index_add_(0, graph, x)
    return out / counts.clamp(min=1).to(x.dtype)[:, None]


@contextlib.contextmanager
def side(name):
    """'hip': the library as it is; 'torch': its two graph operators replaced by the torch restatement."""
    saved = mpnn.aggregate, mpnn.segment_mean
    if name == "torch":
        mpnn.aggregate, mpnn.segment_mean = _torch_aggregate, _torch_segment_mean
    try:
        yield
    finally:
        mpnn.aggregate, mpnn.segment_mean = saved


def mpgnn_epoch_ms(split, x, model, epochs):
    stamps = []

    def on_epoch(_):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())

    torch.cuda.synchronize()
    mpgnn.train(split.edge_index(), x, mpgnn.split_lists(split), model, epochs=epochs, eval_steps=epochs, seed=1,
                num_nodes=split.num_nodes, device=DEV, on_epoch=on_epoch)
    return (np.diff(stamps)[WARM:] * 1e3).tolist()


def seal_sets(split, num_hops=2):
    def prep(name):
        pos, neg = split.links[name]
        li = np.concatenate([pos, neg], axis=1)
        y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(DEV)
        return enclosing_subgraphs(li, split.A, None, 0, num_hops, "drnl"), y

    return prep("train"), prep("test")


def seal_run(sets, model, epochs, seed):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    auc, _ = harness.train_and_evaluate_seal_mpnn(*sets, model=model, hidden=32, num_layers=3, epochs=epochs, lr=1e-3,
                                                  seed=seed)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, auc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "mpgnn_probe.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--thresholds", action="store_true")
    a = ap.parse_args()
    sides = ["hip"] if a.only_hip else ["hip", "torch"]
    n, e = W.load_topology("usair")
    usair = W.edge_split(n, e, seed=1)
    n, e = W.load_topology("cora")
    cora = W.edge_split(n, e, seed=1)
    cora_x = W.normalize_features(W.load_features("cora"))
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "mpgnn_epoch_ms": {}, "seal_epoch_ms": {}}
    for name, split, x in (("usair_eye", usair, None), ("cora_feat", cora, cora_x)):
        for model in ("SAGE", "GIN"):
            ms = {s: [] for s in sides}
            for _ in range(a.reps):                       # alternated: both sides see the same machine state
                for s in sides:
                    with side(s):
                        ms[s] += mpgnn_epoch_ms(split, x, model, 30)
            out["mpgnn_epoch_ms"][f"{name}/{model}"] = {s: statistics.median(v) for s, v in ms.items()}
            print(name, model, out["mpgnn_epoch_ms"][f"{name}/{model}"], flush=True)
    sets = seal_sets(usair)
    for model in ("SAGE", "GIN"):
        ms = {s: [] for s in sides}
        for rep in range(a.reps + 1):
            for s in sides:
                with side(s):
                    t, _ = seal_run(sets, model, 1, 1)
                if rep:                                   # the first round warms both sides up
                    ms[s].append(t)
        out["seal_epoch_ms"][f"usair_2hop/{model}"] = {s: statistics.median(v) for s, v in ms.items()}
        print("seal", model, out["seal_epoch_ms"][f"usair_2hop/{model}"], flush=True)
    if a.thresholds:
        out["auc"] = {}
        for model in ("SAGE", "GIN"):
            for s in sides:
                with side(s):
                    mp = [mpgnn.run_mpgnn(usair, model, None, epochs=50, seed=seed)["AUC"][1] for seed in (1, 2, 3)]
                    sl = [seal_run(sets, model, 4, seed)[1] for seed in (1, 2, 3)]
                out["auc"][f"mpgnn/{model}/{s}"] = mp
                out["auc"][f"seal/{model}/{s}"] = sl
                print("auc", model, s, "mpgnn", mp, "seal", sl, flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
