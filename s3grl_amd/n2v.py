"""The N2V row of the reference's Table 2 (baselines/n2v.py run_n2v): node2vec embeddings trained by `node2vec.Node2Vec`,
and after every evaluated epoch a fresh logistic-regression link classifier (`linkclf.LinkClassifier`) fitted on the
Hadamard features of the train links and read out on valid and test.  Embedding, fit, predictions and confusion counts
stay on the device; per evaluation the host sees θ and eight integers.

    auc = run_n2v(device, data, split_edge, 50, 0.01, 32, 1, 32, 0, args, seed)        # the reference's call
    results = run_n2v_row(split)                                     # {'AUC': (val, test), 'AP': (val, test)}

Two quirks of the reference are kept on purpose:

  * Its metrics are `roc_auc_score` / `average_precision_score` of `clf.predict`, the hard 0/1 predictions, not of a
    probability.  "AUC" is therefore the balanced accuracy (TPR + TNR) / 2 and "AP" is precision · recall +
    (1 − recall) · prevalence (`linkclf.hard_auc_ap`).  `LinkClassifier.decision_function` is there for a real AUC.
  * The walks run on `data.edge_index` exactly as given (`split_edge['train']['edge'].t()`): nothing is made
    symmetric, so a list with one direction per edge gives directed walks.  `node2vec.csr_of` keeps what it is given.

The classifier is the minimiser of sklearn's objective, not lbfgs's stopping point (see linkclf.py), and node2vec's
draws come from the engine's generator (see node2vec.py), so numbers are not bit-equal to a reference run: same
algorithm, same distributions.  Two runs with one seed are bit-identical.  GPU only; no CPU fallback.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .linkclf import LinkClassifier, _check_dim, hard_auc_ap


def _labelled(split_edge, name, num_nodes):
    """`torch.cat([edge, edge_neg])` of one split with its labels.  The reference labels the second half with
    `zeros(edge.size(0))`, which presumes as many negatives as positives; the labels here follow the lists."""
    from .mf import _pairs

    pos = _pairs(split_edge[name]["edge"], num_nodes, f"split_edge['{name}']['edge']")
    neg = _pairs(split_edge[name]["edge_neg"], num_nodes, f"split_edge['{name}']['edge_neg']")
    y = torch.cat([torch.ones(pos.shape[0], dtype=torch.uint8), torch.zeros(neg.shape[0], dtype=torch.uint8)])
    return torch.cat([pos, neg]), y


def _check_split(split_edge):
    for s in ("train", "valid", "test"):
        if s not in split_edge or "edge" not in split_edge[s] or "edge_neg" not in split_edge[s]:
            raise ValueError("split_edge needs train / valid / test, each with 'edge' and 'edge_neg'")


def _train_run(edge_index, num_nodes, split_edge, *, epochs, hidden, neg_ratio, batch_size, lr, eval_steps, seed, device,
               on_eval=None):
    """One run of run_n2v's loop: per-eval results {'AUC': [(val, test)], 'AP': [...]}.  on_eval(epoch, loss, res, n2v,
    clf, lists) sees the trainer and the fitted classifier of that epoch."""
    from .node2vec import Node2Vec

    epochs, eval_steps = int(epochs), int(eval_steps)
    if epochs < 0 or eval_steps < 1:
        raise ValueError("need epochs >= 0 and eval_steps >= 1")
    _check_split(split_edge)
    hidden = _check_dim(hidden)
    lists = {s: _labelled(split_edge, s, num_nodes) for s in ("train", "valid", "test")}
    n2v = Node2Vec(edge_index, num_nodes, hidden, walk_length=20, context_size=10, walks_per_node=10,
                   num_negative_samples=neg_ratio, p=1, q=1, sparse=True, seed=seed, device=device)
    clf = None
    try:
        dev = n2v.engine.device
        lists = {s: (p.to(dev), y.to(dev)) for s, (p, y) in lists.items()}
        table = n2v._table()
        results = {"AUC": [], "AP": []}
        for epoch in range(epochs):                      # the reference counts epochs from 0
            losses = n2v.fit(1, batch_size=batch_size, lr=lr)
            if epoch % eval_steps:
                continue
            clf = LinkClassifier(hidden, device=dev)     # a fresh classifier per evaluation, from θ = 0
            clf.fit(table, *lists["train"])
            auc, ap = {}, {}
            for s in ("valid", "test"):
                auc[s], ap[s] = hard_auc_ap(*clf.confusion(table, *lists[s]))
            res = {"AUC": (auc["valid"], auc["test"]), "AP": (ap["valid"], ap["test"])}
            for key in results:
                results[key].append(res[key])
            if on_eval is not None:
                on_eval(epoch, losses[0] / n2v.steps_per_epoch(batch_size), res, n2v, clf, lists)
            clf.close()
    finally:
        if clf is not None:
            clf.close()
        n2v.close()
    return results


def run_n2v(device, data, split_edge, epochs, lr, hidden_channels, neg_ratio, batch_size, num_threads, args, seed):
    """Reference baselines/n2v.run_n2v: `args.runs` runs (default 1; each with `seed`, as the reference seeds every run
    alike) of `epochs` epochs of node2vec (walk_length 20, context_size 10, walks_per_node 10, neg_ratio negatives,
    loader batches of batch_size, SparseAdam(lr)) on `data.edge_index` over `data.num_nodes` nodes; at every epoch
    with epoch % args.eval_steps == 0 (default 1; epochs count from 0) a default LogisticRegression on
    train.edge ∪ train.edge_neg, then hard-prediction AP and AUC on valid and test.  Returns the test AUC · 100 at the
    first evaluation of maximal validation AUC of the first run, which is what Logger.print_statistics hands back.
    The reference's log lines go to args.res_dir/log.txt only when args.res_dir is set; nothing is printed.
    num_threads (the loader's workers) is accepted and unused."""
    from .gae import best_at_first_max

    runs = int(getattr(args, "runs", 1))
    eval_steps, log_steps = int(getattr(args, "eval_steps", 1)), int(getattr(args, "log_steps", 1))
    if runs < 1 or log_steps < 1 or eval_steps < 1:
        raise ValueError("need runs >= 1, log_steps >= 1 and eval_steps >= 1")
    if int(epochs) < 1:
        raise ValueError("no evaluation ran: epochs < 1")
    if device is not None and torch.device(device).type == "cpu":
        raise RuntimeError("the N2V row needs a HIP device (MI355X); there is no CPU fallback")
    res_dir = getattr(args, "res_dir", "") or ""
    log_file = os.path.join(res_dir, "log.txt") if res_dir else None
    finals = []
    for run in range(runs):
        def on_eval(epoch, loss, res, n2v, clf, lists, run=run):
            if log_file is not None and epoch % log_steps == 0:
                with open(log_file, "a") as f:
                    for key, (v, t) in res.items():
                        print(f"{key}\nRun: {run + 1:02d}, Epoch: {epoch:02d}, Loss: {loss:.4f}, Valid: {100 * v:.2f}%, "
                              f"Test: {100 * t:.2f}%", file=f)

        results = _train_run(data.edge_index, data.num_nodes, split_edge, epochs=epochs, hidden=hidden_channels,
                             neg_ratio=neg_ratio, batch_size=batch_size, lr=lr, eval_steps=eval_steps, seed=seed,
                             device=device, on_eval=on_eval)
        r = (100 * torch.tensor(results["AUC"])).numpy()   # fp32, as Logger.print_statistics
        finals.append(float(best_at_first_max(r)[1]))
    return finals[0]


def run_n2v_row(split, *, epochs=50, hidden=32, neg_ratio=1, batch_size=32, lr=0.01, seed=1, device=None):
    """One Table 2 N2V row from a `workloads.Split` (50 epochs, 32 channels, one negative, batches of 32, lr 0.01,
    eval every epoch; walks on `split_edge['train']['edge'].t()` as given): {'AUC': (best val, test at it), 'AP':
    (...)}, each chosen at the first epoch of its own maximal val value, as fractions (like run_mf)."""
    from .gae import best_at_first_max

    if int(epochs) < 1:
        raise ValueError("epochs must be >= 1")
    split_edge = split.split_edge()
    edge_index = np.ascontiguousarray(np.asarray(split_edge["train"]["edge"]).T)
    results = _train_run(edge_index, split.num_nodes, split_edge, epochs=epochs, hidden=hidden, neg_ratio=neg_ratio,
                         batch_size=batch_size, lr=lr, eval_steps=1, seed=seed, device=device)
    return {k: tuple(float(v) for v in best_at_first_max(r)) for k, r in results.items()}
