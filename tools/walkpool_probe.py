"""WalkPool at its default shape on the GPU (USAir, 2 hops, batch 32, heads 2, walk_len 7, hidden 32): the time of a
training step, of walk_pool forward + backward alone and of its forward alone, beside the same step with the two HIP
operators replaced by a dense torch restatement on the same GPU (padded [B, heads, n_max, n_max] matrices, softmax, bmm
powers).

    python tools/walkpool_probe.py [--out profiles/walkpool_probe.json] [--full-run]

Each figure is the median over `rounds` rounds of the mean over one window of `cycles` passes over the same five
batches (80 steps, 0.3 s and more), between device synchronisations; the variants take turns inside every round, and
one untimed round comes first; min and max of the rounds beside it.  --full-run adds
run_walkpool's default run (50 epochs) on the same split and records its test AUC / AP."""
import argparse
import json
import math
import sys
import time
from pathlib import Path

import numpy as np
import torch
from torch.nn import functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HEADS, WALK_LEN, HIDDEN, BATCH, WIDTH = 2, 7, 32, 32, 32


def dense_features(model, x_out, batch):
    """WalkPooling.forward with dense torch in place of attention_weights and walk_pool."""
    wp = model.wp
    q = wp.lin_key2(F.dropout(F.leaky_relu(wp.lin_key1(x_out), 0.2), 0.5, model.training)).view(-1, HEADS, HIDDEN)
    k = wp.lin_query2(F.dropout(F.leaky_relu(wp.lin_query1(x_out), 0.2), 0.5, model.training)).view(-1, HEADS, HIDDEN)
    ei, mask = batch.in_edge_index()
    B, n = batch.num_graphs, batch.max_nodes
    link = batch.link.long()
    first = batch.node_ptr[:-1][link]
    w = (q[ei[0]] * k[ei[1]]).sum(-1) / math.sqrt(HIDDEN)                        # [e, heads]
    g, r, c = link[ei[1]], ei[0] - first[ei[0]], ei[1] - first[ei[1]]
    dense = torch.full((B, n, n, HEADS), -math.inf, device=w.device).index_put((g, c, r), w)
    Pp = torch.softmax(dense, dim=2).nan_to_num(0.0)                             # rows without an arc: zeros
    keep = torch.ones((B, n, n, 1), device=w.device).index_put((g[~mask], c[~mask], r[~mask]),
                                                               torch.zeros((1,), device=w.device))
    ex = torch.exp(dense - dense.detach().amax(dim=2, keepdim=True).nan_to_num(0.0, neginf=0.0)) * keep
    Pm = ex / (ex.sum(2, keepdim=True) + 1e-16)
    omega = torch.zeros((B, HEADS), device=w.device).index_add(0, g[~mask], torch.sigmoid(w[~mask]))
    Pp, Pm = Pp.permute(0, 3, 1, 2), Pm.permute(0, 3, 1, 2)                      # [B, heads, n, n]
    Xp, Xm, cols = Pp, Pm, []
    for _ in range(WALK_LEN):
        Xp, Xm = Xp @ Pp, Xm @ Pm
        tr = lambda X: X.diagonal(dim1=-2, dim2=-1).sum(-1)                      # noqa: E731
        cols.append(torch.stack([tr(Xp) - tr(Xm), Xp[..., 0, 0] + Xp[..., 1, 1], Xm[..., 0, 0] + Xm[..., 1, 1],
                                 Xp[..., 0, 1] + Xp[..., 1, 0], Xm[..., 0, 1] + Xm[..., 1, 0]], dim=-1))
    walks = torch.stack(cols, dim=2).permute(0, 3, 1, 2).reshape(B, 5, HEADS * WALK_LEN)
    return torch.cat([walks[:, 0], omega, walks[:, 1], walks[:, 2], walks[:, 3], walks[:, 4]], dim=1)


def forward(model, batch, dense):
    x = batch.x
    h1 = model.conv1(x, batch)
    h2 = model.conv2(F.dropout(h1.relu(), 0.5, model.training), batch)
    x_out = torch.cat([x, h1, h2], dim=1)
    feats = dense_features(model, x_out, batch) if dense else model.wp(x_out, batch)
    return model.classifier(feats)


def timed(variants, rounds, cycles):
    """variants: name -> (fn, items).  Every round times each variant once, one after the other (A, B, C, .. , A, B, ..),
    so that drift of the device hits all alike; a window is `cycles` passes over the variant's items."""
    out = {name: [] for name in variants}
    for r in range(rounds + 1):
        for name, (fn, items) in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(cycles):
                for it in items:
                    fn(it)
            torch.cuda.synchronize()
            if r:
                out[name].append((time.perf_counter() - t0) / (cycles * len(items)) * 1e6)
    return {name: {"median_us": round(float(np.median(v)), 1), "min_max_us": [round(min(v), 1), round(max(v), 1)]}
            for name, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cycles", type=int, default=16, help="passes over the five batches per timed window")
    ap.add_argument("--full-run", action="store_true")
    args = ap.parse_args()

    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd import workloads as W
    from s3grl_amd.engine import default_engine
    from s3grl_amd.seal import enclosing_subgraphs
    from s3grl_amd.walkpool import LinkPredTwin, WalkPoolSplit, attention_weights, run_walkpool, walk_pool

    eng = default_engine("cuda:0")
    n, e = W.load_topology("usair")
    split = W.edge_split(n, e, seed=0)
    pos, neg = split.links["train"]
    links = np.concatenate([pos[:, :480], neg[:, :480]], axis=1)
    y_all = torch.cat([torch.ones(480), torch.zeros(480)]).to(eng.device)
    subs = enclosing_subgraphs(links, split.A, torch.ones((n, WIDTH)), 0, 2, "zo", engine=eng)
    wps = WalkPoolSplit(subs)
    order = np.random.default_rng(0).permutation(len(wps))
    batches = [order[i * BATCH:(i + 1) * BATCH] for i in range(5)]
    torch.manual_seed(0)
    model = LinkPredTwin(WIDTH, HIDDEN, HEADS, WALK_LEN, MSE=False).to(eng.device).train()
    opt = torch.optim.Adam(model.parameters(), lr=5e-5)

    def step(ids, dense=False):
        b = wps.batch(ids)
        opt.zero_grad(set_to_none=True)
        loss = F.binary_cross_entropy_with_logits(forward(model, b, dense).view(-1),
                                                  y_all[torch.from_numpy(ids).to(eng.device)])
        loss.backward()
        opt.step()

    fixed = []
    for ids in batches:
        b = wps.batch(ids)
        q = torch.randn((b.num_nodes, HEADS, HIDDEN), device=eng.device)
        k = torch.randn((b.num_nodes, HEADS, HIDDEN), device=eng.device)
        wp_, wm_, _ = attention_weights(q, k, b)
        fixed.append((b, wp_, wm_, torch.randn((len(ids), HEADS, WALK_LEN, 5), device=eng.device)))

    def walk_only(item):
        b, wp_, wm_, g = item
        a, c = wp_.clone().requires_grad_(), wm_.clone().requires_grad_()
        walk_pool(a, c, b, WALK_LEN).backward(g)

    def walk_forward_only(item):
        with torch.no_grad():
            walk_pool(item[1], item[2], item[0], WALK_LEN)

    # the two steps compute the same loss
    model.eval()
    with torch.no_grad():
        b0 = wps.batch(batches[0])
        agree = float((forward(model, b0, False) - forward(model, b0, True)).abs().max())
    model.train()
    counts = subs.node_counts()
    times = timed({"train_step_hip": (step, batches),
                   "train_step_dense_torch": (lambda ids: step(ids, True), batches),
                   "walk_pool_forward_backward_hip": (walk_only, fixed),
                   "walk_pool_forward_hip": (walk_forward_only, fixed)}, args.rounds, args.cycles)
    res = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.cycles * len(batches),
           "shape": {"dataset": "usair", "num_hops": 2, "batch": BATCH, "heads": HEADS, "walk_len": WALK_LEN,
                     "hidden": HIDDEN, "x_width": WIDTH, "links": int(len(wps)),
                     "nodes_per_subgraph_mean_max": [round(float(counts.mean()), 1), int(counts.max())],
                     "arcs_per_subgraph_mean": round(float(np.diff(wps.arc_ptr).mean()), 1)},
           "method": "median over rounds of the mean over one window of reps steps (cycles passes over the same five "
                     "batches), wall clock between device synchronisations; the four variants are timed in turn inside "
                     "every round; one untimed round first",
           "logit_difference_hip_vs_dense": agree, **times}
    if args.full_run:
        t0 = time.perf_counter()
        r = run_walkpool(split, seed=1, device=eng.device)
        res["full_run"] = {"epochs": 50, "seconds": round(time.perf_counter() - t0, 1),
                           "best_val_auc": r["best_val_auc"], "best_val_loss": r["best_val_loss"],
                           "last": r["history"][-1]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
