"""Graph autoencoders (s3grl_amd.gae) on the GPU: warm ms per training epoch and per evaluation, the same epoch done by
a torch-only GPU restatement (index_add propagation, torch negatives, autograd loss) in the same process, alternated
with it, and the 50-epoch val / test AUC of every model, on USAir (x = None), Cora (its bag-of-words rows) and PubMed
(x = None, and the headline's synthetic features).  Writes profiles/gae_probe.json.

    python tools/gae_probe.py [--out FILE] [--reps R] [--only-hip] [--skip-auc]

Run it under `rocprofv3 --kernel-trace --stats` with `--only-hip --skip-auc` for kernel times and launches per epoch.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from s3grl_amd import gae  # noqa: E402
from s3grl_amd import workloads as W  # noqa: E402

DEV = "cuda:0"


def configs():
    n, e = W.load_topology("usair")
    yield "usair_eye", W.edge_split(n, e, seed=0), None
    n, e = W.load_topology("cora")
    yield "cora_feat", W.edge_split(n, e, seed=1), W.normalize_features(W.load_features("cora"))
    n, e = W.load_topology("pubmed")
    sp = W.edge_split(n, e, seed=2)
    yield "pubmed_eye", sp, None
    yield "pubmed_headline_x", sp, W.sparse_uniform_features(n, 500, 50, 2)


class TorchEpoch:
    """The same epoch in torch ops only: propagation by index_add over (src, dst, coef), negatives by rejection of
    uniform draws against the sorted positive keys (3 rounds), the loss by autograd."""

    def __init__(self, ei, n, x, net):
        ei = torch.as_tensor(ei).to(DEV).long()
        keep = ei[0] != ei[1]
        node = torch.arange(n, device=DEV)
        self.src = torch.cat([ei[0][keep], node])
        self.dst = torch.cat([ei[1][keep], node])
        deg = torch.zeros(n, device=DEV).index_add_(0, self.dst, torch.ones_like(self.dst, dtype=torch.float32))
        dinv = deg.pow(-0.5)
        self.coef = dinv[self.src] * dinv[self.dst]
        self.pos = ei
        self.keys = torch.sort(ei[0] * (n - 1) + ei[1] - (ei[1] > ei[0]).long()).values
        self.n, self.x, self.net = n, x, net
        self.opt = torch.optim.Adam(net.encoder.parameters(), lr=0.01)
        self.gen = torch.Generator(device=DEV).manual_seed(0)

    def prop(self, h, b):
        return torch.zeros_like(h).index_add_(0, self.dst, self.coef[:, None] * h[self.src]) + b

    def encode(self):
        e = self.net.encoder
        h = gae._lin(self.x, e.conv1.lin.weight)
        h = self.prop(h, e.conv1.bias).relu()
        if not self.net.variational:
            return self.prop(h @ e.conv2.lin.weight.t(), e.conv2.bias)
        w = torch.cat([e.conv_mu.lin.weight, e.conv_logstd.lin.weight], 0)
        out = self.prop(h @ w.t(), torch.cat([e.conv_mu.bias, e.conv_logstd.bias]))
        mu, ls = out[:, :self.net.out_channels], out[:, self.net.out_channels:].clamp(max=10)
        return mu + torch.randn(mu.shape, generator=self.gen, device=DEV) * torch.exp(ls)

    def negatives(self):
        n, m = self.n, self.keys.numel()
        count = m + n
        pop = n * (n - 1)
        size = int(1.1 * count / (1 - m / pop))
        got = None
        for _ in range(3):
            r = torch.randint(0, pop, (size,), generator=self.gen, device=DEV).unique()
            r = r[~torch.isin(r, self.keys)]
            if got is not None:
                r = r[~torch.isin(r, got)]
            got = r if got is None else torch.cat([got, r])
            if got.numel() >= count:
                break
        got = got[:count]
        i = torch.div(got, n - 1, rounding_mode="floor")
        j = got % (n - 1)
        return torch.stack([i, j + (j >= i).long()])

    def epoch(self):
        self.opt.zero_grad(set_to_none=True)
        z = self.encode()
        neg = self.negatives()
        lp = (z[self.pos[0]] * z[self.pos[1]]).sum(1)
        ln = (z[neg[0]] * z[neg[1]]).sum(1)
        loss = -torch.log(torch.sigmoid(lp) + 1e-15).mean() - torch.log(1 - torch.sigmoid(ln) + 1e-15).mean()
        loss.backward()
        self.opt.step()


class HipEpoch:
    def __init__(self, split, x, model):
        n = split.num_nodes
        self.x = None if x is None else torch.as_tensor(x).to(DEV).contiguous()
        self.net = gae.TWINS[model](n if x is None else x.shape[1], 32, 64, seed=1).to(DEV)
        ei = split.edge_index()
        self.graph = gae.GcnGraph(ei, n, DEV)
        self.pos = gae.PairList(ei, n, DEV)
        self.pos.keys()
        self.pos.incidence()
        self.opt = torch.optim.Adam(self.net.encoder.parameters(), lr=0.01)
        lists = {"val": split.links["valid"], "test": split.links["test"]}
        self.lists = {k: (gae.PairList(p, n, DEV), gae.PairList(q, n, DEV)) for k, (p, q) in lists.items()}
        self.e = 0

    def epoch(self):
        self.e += 1
        self.net.train()
        self.opt.zero_grad(set_to_none=True)
        z = self.net.encode(self.x, self.graph)
        loss = self.net.recon_loss(z, self.pos, gae.recon_negatives(self.pos, 1, self.e))
        loss.backward()
        self.opt.step()

    def evaluate(self):
        self.net.eval()
        with torch.no_grad():
            z = self.net.encode(self.x, self.graph)
        return gae._evaluate(z, self.lists)


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "gae_probe.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--skip-auc", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "configs": {}}
    for name, split, x in configs():
        row = {"num_nodes": split.num_nodes, "train_pairs": int(split.edge_index().shape[1]),
               "features": None if x is None else int(x.shape[1])}
        for model in gae.MODELS:
            hip = HipEpoch(split, x, model)
            tor = None if a.only_hip else TorchEpoch(split.edge_index(), split.num_nodes, hip.x,
                                                     gae.TWINS[model](hip.net.in_channels, 32, 64, seed=1).to(DEV))
            for _ in range(3):
                hip.epoch()
                if tor:
                    tor.epoch()
            th, tt = [], []
            for _ in range(a.reps):   # alternated
                th += timed(hip.epoch, 1)
                if tor:
                    tt += timed(tor.epoch, 1)
            te = timed(hip.evaluate, max(3, a.reps // 4))
            m = {"hip_epoch_ms_median": float(np.median(th)), "hip_epoch_ms_min": float(np.min(th)),
                 "eval_ms_median": float(np.median(te))}
            if tor:
                m["torch_epoch_ms_median"] = float(np.median(tt))
                m["torch_epoch_ms_min"] = float(np.min(tt))
            if not a.skip_auc:
                r = gae.run_gae(split, model, x=None if x is None else torch.as_tensor(x), device=DEV)
                m["val_auc"], m["test_auc"] = r["AUC"]
                m["val_ap"], m["test_ap"] = r["AP"]
            row[model] = m
            print(name, model, json.dumps(m), flush=True)
        res["configs"][name] = row
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
