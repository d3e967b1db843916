"""Fused SIGNNet trainer probe: µs per step and seconds per epoch of `SIGNNetTrainer.fit_epoch` and of
the eager loop of `harness.train_and_evaluate` (its training part, written out here step for step) on the same GPU, on
the train split of USAir PoS sign_k=2 (in_width 51) and of PubMed PoS sign_k=3 (in_width 2004), hidden 256, batches
of 32, dropout 0.5.  Host clock from the first call to the read-back of the last epoch's losses, after a warm-up epoch
on a trainer (a model) of its own; seeds 1, 2, 3.

    python tools/signnet_probe.py [--out profiles/signnet_probe.json] [--epochs 3] [--eager-epochs 1] [--only-engine NAME]

`--only-engine NAME` runs nothing but the fused epochs of one workload: the run to put under `rocprofv3 --kernel-trace
--stats` for the kernel split of a step.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
from torch import nn

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

CFG = dict(hidden=256, batch_size=32, dropout=0.5, lr=1e-4)
WORKLOADS = ("usair_pos_k2", "pubmed_pos_k3")


def train_split(name):
    """(rows, row_ptr, y) of the workload's train split on the device, and the precompute's seconds."""
    from s3grl_amd import workloads
    from s3grl_amd.engine import Engine

    w = workloads.make(name)
    eng = Engine("cuda:0")
    G, f = eng.graph(w.A), eng.features(w.X)
    pos, neg = w.split.links["train"]
    li = np.concatenate([pos, neg], axis=1)
    y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
    links = eng.links(li)
    eng.precompute(G, f, links, mode=w.mode, num_hops=w.num_hops, sign_k=w.sign_k)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = eng.precompute(G, f, links, mode=w.mode, num_hops=w.num_hops, sign_k=w.sign_k)
    torch.cuda.synchronize()
    return (res.rows, res.row_ptr, y), time.perf_counter() - t0, eng


def fused_epochs(train, seed, epochs):
    """Seconds of `epochs` fused epochs, from the first call to the read-back of the last epoch's losses."""
    from s3grl_amd.signnet import SIGNNetTrainer

    rows, row_ptr, y = train
    net = SIGNNetTrainer(rows.shape[1] * rows.shape[2], CFG["hidden"], dropout=CFG["dropout"], lr=CFG["lr"], seed=seed)
    rows, row_ptr, y = net._store(rows, row_ptr, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = [net._epoch(rows, row_ptr, y, CFG["batch_size"]) for _ in range(epochs)]
    last = losses[-1].cpu()
    spent = time.perf_counter() - t0
    net.close()
    return spent, float(last.mean())


def eager_epochs(train, seed, epochs):
    """Seconds of `epochs` epochs of harness.train_and_evaluate's training loop, ending in a read-back of the loss."""
    from s3grl_amd.harness import RowCounts, SIGNNetTwin, batch_slices

    torch.manual_seed(seed)
    rows, row_ptr, y = train
    dev = rows.device
    model = SIGNNetTwin(rows.shape[1] * rows.shape[2], CFG["hidden"], 0, "", CFG["dropout"]).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=CFG["lr"])
    L, yf, counts, bs = y.numel(), y.float(), RowCounts(row_ptr), CFG["batch_size"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        model.train()
        perm = torch.randperm(L)
        for b in range(0, L - 1, bs):
            ids_h = perm[b:b + bs]
            ids = ids_h.to(dev, non_blocking=True)
            idx, local = batch_slices(row_ptr, ids, counts.total(ids_h))
            loss = nn.functional.binary_cross_entropy_with_logits(model(rows[idx], local), yf[ids])
            opt.zero_grad()
            loss.backward()
            opt.step()
    last = float(loss.detach())
    return time.perf_counter() - t0, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "signnet_probe.json"))
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--eager-epochs", type=int, default=1)
    ap.add_argument("--only-engine", default="")
    a = ap.parse_args()
    if a.only_engine:
        train, _, eng = train_split(a.only_engine)
        fused_epochs(train, 0, 1)
        print(json.dumps({"fused_epochs_s": fused_epochs(train, 1, a.epochs)[0], "epochs": a.epochs}))
        eng.close()
        return
    res = {"config": CFG, "workloads": {}}
    for name in WORKLOADS:
        train, pre_s, eng = train_split(name)
        L = train[2].numel()
        steps = -(-(L - 1) // CFG["batch_size"])
        fused_epochs(train, 0, 1)                                       # warm-up: code objects, allocator
        fused = [fused_epochs(train, s, a.epochs) for s in (1, 2, 3)]
        eager_epochs(train, 0, 1) if name == WORKLOADS[0] else None      # warm-up of torch's kernels
        eager = [eager_epochs(train, s, a.eager_epochs) for s in (1, 2, 3)]
        fs, es = float(np.median([r[0] for r in fused])) / a.epochs, float(np.median([r[0] for r in eager])) / a.eager_epochs
        res["workloads"][name] = {
            "links": L, "rows": int(train[0].shape[0]), "in_width": int(train[0].shape[1] * train[0].shape[2]),
            "steps_per_epoch": steps, "precompute_s": pre_s,
            "fused_epochs_timed": a.epochs, "fused_s": [r[0] for r in fused], "fused_s_per_epoch": fs,
            "fused_us_per_step": 1e6 * fs / steps, "fused_last_epoch_mean_loss": [r[1] for r in fused],
            "eager_epochs_timed": a.eager_epochs, "eager_s": [r[0] for r in eager], "eager_s_per_epoch": es,
            "eager_us_per_step": 1e6 * es / steps, "eager_last_loss": [r[1] for r in eager],
            "eager_over_fused": es / fs}
        del train
        eng.close()
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
