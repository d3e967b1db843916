"""MF baseline probe:
  * 50 epochs of run_MF's loop (hidden 32, 3 layers, dropout 0.5, batches of 32, Adam lr 0.01) on the engine, on the
    USAir train split and on Router (tests/golden/router_edges.txt, split the same way): host clock around the 50
    epochs ending in a device read-back, after a warm-up epoch on a trainer of its own, three seeds; µs per step
  * the same loop as eager torch (`torch_mf`, the reference's structure written afresh) on the same GPU and on the
    CPU threads torch is given (a few epochs, scaled)
  * test AUC of the engine and of the eager-torch loop on USAir, seeds 1, 2, 3 (`--auc`; CPU only with `--cpu-only`)

    python tools/mf_probe.py [--out profiles/mf_probe.json] [--torch-epochs 3] [--auc] [--cpu-only] [--only-engine]

`--only-engine` runs nothing but the engine's 50 epochs on USAir: the run to put under `rocprofv3 --kernel-trace
--stats` for the kernel split of a step.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

CFG = dict(hidden=32, num_layers=3, dropout=0.5, batch_size=32, lr=0.01, epochs=50)


def splits():
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    out = {"usair_train": W.edge_split(n, e, seed=0)}
    n_r, e_r = W.read_seal_edges(REPO / "tests" / "golden" / "router_edges.txt")
    out["router"] = W.edge_split(n_r, W.undirected_unique(e_r), seed=0)
    return out


class TorchMF(torch.nn.Module):
    def __init__(self, n, hidden, num_layers, dropout):
        super().__init__()
        self.emb = torch.nn.Embedding(n, hidden)
        self.lins = torch.nn.ModuleList([torch.nn.Linear(hidden, hidden) for _ in range(num_layers - 1)] +
                                        [torch.nn.Linear(hidden, 1)])
        self.dropout = dropout

    def forward(self, pairs):
        x = self.emb.weight
        h = x[pairs[:, 0]] * x[pairs[:, 1]]
        for lin in self.lins[:-1]:
            h = F.dropout(F.relu(lin(h)), p=self.dropout, training=self.training)
        return torch.sigmoid(self.lins[-1](h))[:, 0]


def torch_epoch(net, opt, train, batch_size, n):
    net.train()
    total = 0.0
    perm = torch.randperm(train.shape[0], device=train.device)
    for i in range(0, train.shape[0], batch_size):
        opt.zero_grad()
        pos = train[perm[i:i + batch_size]]
        neg = torch.randint(0, n, pos.shape, dtype=torch.long, device=train.device)
        loss = -torch.log(net(pos) + 1e-15).mean() + -torch.log(1 - net(neg) + 1e-15).mean()
        loss.backward()
        opt.step()
        total += loss.detach() * pos.shape[0]
    return float(total) / train.shape[0]


def torch_mf(split, seed, device, epochs=None, evaluate=True):
    """The eager-torch loop: ({'AUC': (val, test), 'AP': ...} or None, seconds of the epochs alone)."""
    from s3grl_amd.gae import best_at_first_max
    from s3grl_amd.heuristics import average_precision, roc_auc

    torch.manual_seed(seed)
    se = split.split_edge()
    dev = torch.device(device)
    net = TorchMF(split.num_nodes, CFG["hidden"], CFG["num_layers"], CFG["dropout"]).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=CFG["lr"])
    train = torch.as_tensor(se["train"]["edge"]).to(dev)
    results = {"AUC": [], "AP": []}
    spent = 0.0
    for _ in range(CFG["epochs"] if epochs is None else epochs):
        t0 = time.perf_counter()
        torch_epoch(net, opt, train, CFG["batch_size"], split.num_nodes)   # ends in a read-back of the loss
        spent += time.perf_counter() - t0
        if evaluate:
            net.eval()
            out = {}
            with torch.no_grad():
                for s in ("valid", "test"):
                    pos, neg = (torch.as_tensor(se[s][k]).to(dev) for k in ("edge", "edge_neg"))
                    sc = torch.cat([net(pos), net(neg)]).cpu().numpy()
                    y = np.r_[np.ones(len(pos)), np.zeros(len(neg))]
                    out[s] = (roc_auc(y, sc), average_precision(y, sc))
            results["AUC"].append((out["valid"][0], out["test"][0]))
            results["AP"].append((out["valid"][1], out["test"][1]))
    if not evaluate:
        return None, spent
    return {k: tuple(float(v) for v in best_at_first_max(r)) for k, r in results.items()}, spent


def engine_epochs(split, seed, epochs):
    """Seconds of `epochs` engine epochs, from the first call to the read-back of the last epoch's losses."""
    from s3grl_amd.mf import MFTrainer

    mf = MFTrainer(split.num_nodes, CFG["hidden"], CFG["num_layers"], CFG["dropout"], CFG["lr"], seed=seed)
    train = mf._train_list(split.split_edge()["train"]["edge"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = [mf._epoch(train, CFG["batch_size"]) for _ in range(epochs)]   # each ends in a device read-back
    spent = time.perf_counter() - t0
    mf.close()
    return spent, losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "mf_probe.json"))
    ap.add_argument("--torch-epochs", type=int, default=3)
    ap.add_argument("--auc", action="store_true")
    ap.add_argument("--cpu-only", action="store_true")
    ap.add_argument("--only-engine", action="store_true")
    a = ap.parse_args()
    sp = splits()
    if a.only_engine:
        engine_epochs(sp["usair_train"], 0, 1)
        print(json.dumps({"engine_50_epochs_s": engine_epochs(sp["usair_train"], 1, CFG["epochs"])[0]}))
        return
    res = {"config": CFG, "graphs": {}, "cpu_threads": torch.get_num_threads()}
    if a.auc:
        usair = sp["usair_train"]
        res["torch_cpu_auc_usair_seeds_1_2_3"] = [torch_mf(usair, s, "cpu")[0] for s in (1, 2, 3)]
        if not a.cpu_only:
            from s3grl_amd.mf import run_mf

            res["engine_auc_usair_seeds_1_2_3"] = [run_mf(usair, seed=s) for s in (1, 2, 3)]
    if not a.cpu_only:
        for name, split in sp.items():
            E = split.links["train"][0].shape[1]
            steps = -(-E // CFG["batch_size"])
            engine_epochs(split, 0, 1)                                     # warm-up: code objects, allocator
            runs = [engine_epochs(split, s, CFG["epochs"]) for s in (1, 2, 3)]
            g = {"num_nodes": split.num_nodes, "train_pairs": E, "steps_per_epoch": steps,
                 "engine_50_epochs_s": [r[0] for r in runs],
                 "engine_us_per_step": 1e6 * float(np.median([r[0] for r in runs])) / (CFG["epochs"] * steps),
                 "engine_epoch_losses": runs[0][1][:3] + runs[0][1][-1:]}
            torch_mf(split, 0, "cuda", epochs=1, evaluate=False)           # warm-up
            tg = [torch_mf(split, s, "cuda", epochs=a.torch_epochs, evaluate=False)[1] for s in (1, 2, 3)]
            tc = [torch_mf(split, s, "cpu", epochs=a.torch_epochs, evaluate=False)[1] for s in (1, 2, 3)]
            g["torch_epochs_timed"] = a.torch_epochs
            g["torch_gpu_50_epochs_s_scaled"] = [t * CFG["epochs"] / a.torch_epochs for t in tg]
            g["torch_gpu_us_per_step"] = 1e6 * float(np.median(tg)) / (a.torch_epochs * steps)
            g["torch_cpu_50_epochs_s_scaled"] = [t * CFG["epochs"] / a.torch_epochs for t in tc]
            g["torch_cpu_us_per_step"] = 1e6 * float(np.median(tc)) / (a.torch_epochs * steps)
            res["graphs"][name] = g
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res)[:3000])


if __name__ == "__main__":
    main()
