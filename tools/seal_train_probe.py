"""One training epoch of the SEAL DGCNN twin (s3grl_amd.seal_nn) on two table-2 shapes, timed with a device
synchronise after warm-up epochs, twice in the same run: with the HIP operators, and with the test
restatement's torch ops (tests/seal_nn_reference.py: gcn_norm + index_add propagation per layer call, as
PyG's GCNConv does, and a device-side stable-sort global_sort_pool) in their place.

    python tools/seal_train_probe.py --out DIR            # one JSON line per shape and path, also DIR/seal_train_probe.json
    python tools/seal_train_probe.py --paths hip --warmup 0 --epochs 1   # under rocprofv3 --kernel-trace --stats

Shapes: USAir DGCNN 2-hop drnl, hidden 32, 3 layers, k 0.6; Cora DGCNN 3-hop drnl, hidden 256, 3 layers, k 0.6,
use_feature on Cora's own (normalised) features.  Train links: s3grl_amd.workloads.edge_split (seed 0), train
positives and negatives; batches of 32, Adam at lr 1e-4.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

SHAPES = [("usair", 2, 32, False), ("cora", 3, 256, True)]


def torch_ops():
    """The restatement's operators with the signatures of seal_nn.gcn_propagate / sort_pool (fp32 on the device)."""
    import seal_nn_reference as R

    def gcn_propagate(h, batch, bias=None):
        ew = batch.edge_weight if batch.gcn.use_edge_weight else None
        src, dst, coef = R.gcn_norm(batch.edge_index, batch.num_nodes, ew)
        out = R.propagate(h, src, dst, coef.float())
        return out + bias if bias is not None else out

    def sort_pool(x, node_ptr, k, max_nodes=None, lds_budget=0, return_index=False):
        out, index = R.sort_pool(x, node_ptr, k, R.sort_order_torch(x, node_ptr, k))
        return (out, index) if return_index else out

    return gcn_propagate, sort_pool


def run_shape(eng, name, hops, hidden, use_feature, paths, warmup, epochs):
    import numpy as np
    import torch

    from s3grl_amd import seal_nn
    from s3grl_amd import workloads as W
    from s3grl_amd.seal import enclosing_subgraphs

    n, e = W.load_topology(name)
    sp = W.edge_split(n, e, seed=0)
    x = W.normalize_features(W.load_features(name)) if use_feature else None
    pos, neg = sp.links["train"]
    li = np.concatenate([pos, neg], axis=1)
    y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
    torch.cuda.synchronize()
    t = time.perf_counter()
    subs = enclosing_subgraphs(li, sp.A, x, 0, hops, "drnl", engine=eng)
    subs.gcn_split()
    torch.cuda.synchronize()
    prep_s = time.perf_counter() - t
    hip_ops = (seal_nn.gcn_propagate, seal_nn.sort_pool)
    results = []
    for path in paths:
        seal_nn.gcn_propagate, seal_nn.sort_pool = hip_ops if path == "hip" else torch_ops()
        try:
            torch.manual_seed(0)
            model = seal_nn.DGCNNTwin(hidden, 3, 1000, 0.6, train_dataset=subs, use_feature=use_feature).to(eng.device)
            opt = torch.optim.Adam(model.parameters(), lr=1e-4)
            rng = np.random.default_rng(0)
            times = []
            for ep in range(warmup + epochs):
                model.train()
                perm = rng.permutation(len(subs))
                torch.cuda.synchronize()
                t = time.perf_counter()
                for b in range(0, len(subs), 32):
                    ids = perm[b:b + 32]
                    if ids.size < 2:
                        continue
                    batch = subs.batch(ids)
                    loss = torch.nn.functional.binary_cross_entropy_with_logits(
                        model(batch).view(-1), y[batch.link_ids_device])
                    opt.zero_grad()
                    loss.backward()
                    opt.step()
                torch.cuda.synchronize()
                if ep >= warmup:
                    times.append(time.perf_counter() - t)
        finally:
            seal_nn.gcn_propagate, seal_nn.sort_pool = hip_ops
        counts = subs.node_counts()
        r = {"shape": f"{name} DGCNN {hops}-hop drnl hidden {hidden}" + (" use_feature" if use_feature else ""),
             "path": path, "links": len(subs), "batches": (len(subs) + 31) // 32, "k": model.k,
             "nodes": int(counts.sum()), "max_nodes": int(counts.max()), "edges": int(subs._edge_ptr[-1]),
             "subgraphs_and_split_s": round(prep_s, 3), "warmup_epochs": warmup,
             "epoch_s": [round(v, 4) for v in times], "best_epoch_s": round(min(times), 4)}
        print(json.dumps(r), flush=True)
        results.append(r)
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--paths", default="hip,torch")
    ap.add_argument("--shapes", default="usair,cora")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=2)
    args = ap.parse_args()
    import torch

    from s3grl_amd.engine import Engine

    if not torch.cuda.is_available():
        sys.exit("seal_train_probe needs the MI355X")
    if args.epochs < 1:
        sys.exit("--epochs must be >= 1")
    eng = Engine("cuda:0")
    paths = args.paths.split(",")
    results = []
    for name, hops, hidden, use_feature in SHAPES:
        if name in args.shapes.split(","):
            results += run_shape(eng, name, hops, hidden, use_feature, paths, args.warmup, args.epochs)
    eng.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        Path(args.out, "seal_train_probe.json").write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
