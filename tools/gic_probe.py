#!/usr/bin/env python3
"""Times Graph InfoClust on the GPU: one training epoch (forward, loss, its read on the host as CalGIC's step rule
needs it every epoch, backward, Adam step) and one Clusterator
forward + backward, at the reference's three configurations (N, K, beta of Cora, PubMed and USAir on their train
graphs), each at d = 32 and d = 256, for the HIP path (`s3grl_amd.gic`) and for the same epoch written with plain torch
ops on the same GPU (sparse operator, the reference's cluster() loop): what a user would run without `s3grl_amd.gic`.
Warm-up first, then the two alternate in rounds; the median round is reported.  Writes profiles/gic_probe.json.

    python tools/gic_probe.py
    rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/gic -o gic -- python tools/gic_probe.py --only-hip --config cora --dim 32
        (its <..>_kernel_stats.csv is the record kept as profiles/gic_kernel_stats.csv)
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from s3grl_amd import gic, workloads  # noqa: E402
from s3grl_amd.propagate import GicGraph, gic_arcs  # noqa: E402

DEV = "cuda"
FEATURES = {"cora": 1433, "pubmed": 500, "usair": None}


def torch_cluster(data, init, beta, num_iter):
    mu = init
    data = data / (data.norm(dim=1)[:, None] + 1e-6)
    for _ in range(num_iter):
        mu = mu / (mu.norm(dim=1)[:, None] + 1e-6)
        dist = data @ mu.t()
        r = F.softmax(beta * dist, dim=1)
        mu = torch.diag(1 / r.sum(dim=0)) @ (r.t() @ data)
    return mu, F.softmax(beta * dist, dim=1)


def torch_clusterator(h, init, beta):
    mu, _ = torch_cluster(h, init, beta, 10)
    return torch_cluster(h, mu.clone().detach(), beta, 1)


def torch_forward(net, x, idx, adj, beta):
    """models/gic.py:GIC.forward as the reference runs it: two encoder passes, the dense c2."""
    w = net.gcn.fc.weight
    enc = lambda f: net.gcn.act(torch.sparse.mm(adj, f @ w.t()) + net.gcn.bias)  # noqa: E731
    h1, h2 = enc(x), enc(x[idx])
    Z, S = torch_clusterator(h1, net.init, beta)
    c2 = torch.sigmoid(S @ Z)
    c = torch.sigmoid(h1.mean(0))
    v = net.disc.f_k.weight[0] @ c
    logits = torch.cat([h1 @ v, h2 @ v]) + net.disc.f_k.bias
    return logits[None], torch.cat([(h1 * c2).sum(1), (h2 * c2).sum(1)])[None]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # microseconds per call


def probe(name, dim, reps, rounds, only_hip):
    n, e = workloads.load_topology(name)
    split = workloads.edge_split(n, e, seed=1)
    ei = torch.as_tensor(split.edge_index())
    beta, alpha, K = gic.hyper_parameters(name)
    f = FEATURES[name]
    gen = torch.Generator().manual_seed(0)
    x = None if f is None else torch.rand((n, f), generator=gen).to(DEV)
    graph = GicGraph(ei, n, DEV)
    s, t, coef = gic_arcs(ei[0].to(DEV), ei[1].to(DEV), n)
    adj = torch.sparse_coo_tensor(torch.stack([t, s]), coef.float(), (n, n)).coalesce()
    x_dense = torch.eye(n, device=DEV) if x is None else x          # the reference's x for a featureless graph
    nets = {k: gic.GICTwin(n, n if f is None else f, dim, K, beta, seed=0).to(DEV) for k in ("hip", "torch")}
    opts = {k: torch.optim.Adam(v.parameters(), lr=0.01) for k, v in nets.items()}
    idx = torch.randperm(n, generator=gen).to(DEV)
    h = torch.randn((n, dim), generator=gen).to(DEV)

    def epoch(kind):
        net, opt = nets[kind], opts[kind]
        opt.zero_grad(set_to_none=True)
        out = net(x, idx, graph, beta) if kind == "hip" else torch_forward(net, x_dense, idx, adj, beta)
        loss = gic.gic_loss(out[0], out[1], alpha)
        float(loss.detach())                         # the loop's `if loss < best`: a host read every epoch
        loss.backward()
        opt.step()

    def clusterator(kind):
        hh = h.clone().requires_grad_(True)
        Z, S = (gic.clusterator if kind == "hip" else torch_clusterator)(hh, nets[kind].init, beta)
        (Z.sum() + (S * S).sum()).backward()

    kinds = ("hip",) if only_hip else ("hip", "torch")
    res = {"N": n, "arcs": int(ei.shape[1]), "K": K, "beta": beta, "d": dim, "features": f}
    for what, fn in (("epoch", epoch), ("clusterator", clusterator)):
        for k in kinds:
            for _ in range(3):
                fn(k)
        torch.cuda.synchronize()
        times = {k: [] for k in kinds}
        for _ in range(rounds):
            for k in kinds:
                times[k].append(timed(lambda: fn(k), reps))
        for k in kinds:
            res[f"{what}_{k}_us"] = round(statistics.median(times[k]), 1)
            res[f"{what}_{k}_us_min_max"] = [round(min(times[k]), 1), round(max(times[k]), 1)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "gic_probe.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--config", choices=sorted(FEATURES))
    ap.add_argument("--dim", type=int)
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds, "configs": {}}
    for name in ([a.config] if a.config else ["usair", "cora", "pubmed"]):
        for dim in ([a.dim] if a.dim else [32, 256]):
            res["configs"][f"{name}_d{dim}"] = r = probe(name, dim, a.reps, a.rounds, a.only_hip)
            print(json.dumps({f"{name}_d{dim}": r}), flush=True)
    if not a.only_hip and not a.config and not a.dim:
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
