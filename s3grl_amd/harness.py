"""Thin end-to-end harness for the downstream step: a SIGNNet twin that
consumes the engine's collated output directly on the device — no per-link Python objects, no
host sync in the pooling — and a train / evaluate loop shaped like the reference's
(`train_bce` sgrl_link_pred.py:440-472, `test` :538-587, AUC :704-770).

The model mirrors reference models.py:301-383: `operator_diff` = Linear -> ELU -> BatchNorm ->
dropout over the concatenated operators (PyG MLP with act_first, plain_last=False), centre /
common-neighbour pooling (`s3grl_amd.pool.centre_pool`, HIP kernels), `link_pred_mlp` = Linear
-> ReLU -> BatchNorm -> dropout -> Linear.  It exists to show that what the engine emits is what
the reference's MLP consumes; it is plain PyTorch apart from the pooling.
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .pool import centre_pool


class SIGNNetTwin(nn.Module):
    def __init__(self, in_width, hidden=256, k_heuristic=0, k_pool_strategy="", dropout=0.5):
        """in_width = (sign_k + 1) * (1 + F): one collated row (reference models.py:316-320)."""
        super().__init__()
        self.k_heuristic, self.k_pool_strategy = k_heuristic, k_pool_strategy
        self.operator_diff = nn.Sequential(nn.Linear(in_width, hidden), nn.ELU(),
                                           nn.BatchNorm1d(hidden), nn.Dropout(dropout))
        # reference models.py:327-337: hidden x 2 for mean / sum pooling of the common-neighbour rows,
        # hidden x (1 + k_heuristic) when they are concatenated, hidden alone without the heuristic
        if not k_heuristic:
            ch = 1
        elif k_pool_strategy == "concat":
            ch = 1 + int(k_heuristic)
        else:
            ch = 2
        self.link_pred_mlp = nn.Sequential(nn.Linear(hidden * ch, hidden), nn.ReLU(),
                                           nn.BatchNorm1d(hidden), nn.Dropout(dropout),
                                           nn.Linear(hidden, 1))

    def forward(self, rows, row_ptr):
        """rows [ΣR_b, K+1, 1+F] of the links of one mini-batch, row_ptr [B+1] local to it."""
        h = self.operator_diff(rows.reshape(rows.shape[0], -1))
        z = centre_pool(h, row_ptr, self.k_heuristic, self.k_pool_strategy)
        return self.link_pred_mlp(z).view(-1)


def batch_slices(row_ptr, link_ids, total=None):
    """Device-side gather of the rows of a set of links: (row index [ΣR_b], local row_ptr [B+1]).
    `total` = ΣR_b when the caller knows it on the host (`RowCounts`): then nothing here waits for
    the device; without it the size is read back (one sync)."""
    start, end = row_ptr[link_ids], row_ptr[link_ids + 1]
    cnt = end - start
    local = torch.zeros(link_ids.numel() + 1, dtype=torch.int64, device=row_ptr.device)
    local[1:] = torch.cumsum(cnt, 0)
    if total is None:
        total = int(local[-1])
    idx = torch.repeat_interleave(start - local[:-1], cnt, output_size=total) + torch.arange(
        total, device=row_ptr.device)
    return idx, local


class RowCounts:
    """Rows per link on the HOST, fetched once per dataset: the loader draws its mini-batches on the
    host (like the reference's DataLoader) and knows every batch's row total without asking the
    device — no host sync per mini-batch (the reference has one per batch, models.py:341)."""

    def __init__(self, row_ptr):
        self.counts = (row_ptr[1:] - row_ptr[:-1]).cpu()

    def total(self, link_ids_host):
        return int(self.counts[link_ids_host].sum())


def auc_score(scores, labels):
    """Rank-based AUC (ties averaged), on the device."""
    s = scores.double()
    order = torch.argsort(s)
    ranks = torch.empty_like(s)
    ranks[order] = torch.arange(1, s.numel() + 1, dtype=torch.float64, device=s.device)
    # average ranks of ties
    uniq, inv, cnt = torch.unique(s, return_inverse=True, return_counts=True)
    sums = torch.zeros_like(uniq).scatter_add_(0, inv, ranks)
    ranks = (sums / cnt.double())[inv]
    pos = labels > 0
    n_pos, n_neg = int(pos.sum()), int((~pos).sum())
    return float((ranks[pos].sum() - n_pos * (n_pos + 1) / 2) / max(n_pos * n_neg, 1))


def train_and_evaluate(train, test, *, k_heuristic=0, k_pool_strategy="", hidden=256, epochs=10,
                       batch_size=32, lr=1e-3, seed=0, dropout=0.5):
    """train / test: (rows, row_ptr, y) device tensors as `Engine.precompute` returns them."""
    torch.manual_seed(seed)
    rows, row_ptr, y = train
    dev = rows.device
    model = SIGNNetTwin(rows.shape[1] * rows.shape[2], hidden, k_heuristic, k_pool_strategy,
                        dropout).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    L = y.numel()
    yf = y.float()
    counts = RowCounts(row_ptr)
    for _ in range(epochs):
        model.train()
        perm = torch.randperm(L)
        for b in range(0, L - 1, batch_size):
            ids_h = perm[b:b + batch_size]
            if ids_h.numel() < 2:
                continue
            ids = ids_h.to(dev, non_blocking=True)
            idx, local = batch_slices(row_ptr, ids, counts.total(ids_h))
            loss = nn.functional.binary_cross_entropy_with_logits(model(rows[idx], local), yf[ids])
            opt.zero_grad()
            loss.backward()
            opt.step()
    model.eval()
    rows_t, ptr_t, y_t = test
    out = []
    counts_t = RowCounts(ptr_t)
    with torch.no_grad():
        for b in range(0, y_t.numel(), 1024):
            ids_h = torch.arange(b, min(b + 1024, y_t.numel()))
            ids = ids_h.to(dev, non_blocking=True)
            idx, local = batch_slices(ptr_t, ids, counts_t.total(ids_h))
            out.append(model(rows_t[idx], local))
    return auc_score(torch.cat(out), y_t), model


def train_and_evaluate_fused(train, test, *, k_heuristic=0, k_pool_strategy="", hidden=256, epochs=10,
                             batch_size=32, lr=1e-3, seed=0, dropout=0.5):
    """`train_and_evaluate` on the fused HIP trainer (`s3grl_amd.signnet.SIGNNetTrainer`): the same model, loss,
    optimiser and batching, every mini-batch step four kernel launches reading the links' rows in place, one wait
    per epoch.  Draws come from the engine's counter-based generator, not torch's streams, so for one seed the two
    functions give different (equally distributed) runs.  Returns (test AUC, trainer); `trainer.state_dict()`
    loads into a `SIGNNetTwin`."""
    from .signnet import SIGNNetTrainer

    rows, row_ptr, y = train
    net = SIGNNetTrainer(rows.shape[1] * rows.shape[2], hidden, k_heuristic, k_pool_strategy, dropout, lr, seed=seed,
                         device=rows.device)
    rows, row_ptr, yf = net._store(rows, row_ptr, y)
    for _ in range(epochs):
        net._epoch(rows, row_ptr, yf, batch_size)
    rows_t, ptr_t, y_t = test
    return auc_score(net.score(rows_t, ptr_t), y_t), net


EVAL_METRICS = ("auc", "rocauc", "hits", "mrr")


def _epoch_metric(metrics, eval_metric, scores, split):
    """One split's results of one epoch: {key: value}.  split: (labels, positive ids, negative ids) on the device."""
    y, pos, neg = split
    if eval_metric == "auc":
        r = metrics.ranked(scores, y)
        return {"AUC": r["AUC"], "AP": r["AP"]}
    if eval_metric == "rocauc":
        return {"rocauc": metrics.ranked(scores, y)["AUC"]}
    if eval_metric == "hits":
        r = metrics.ranked(scores, y, ks=(20, 50, 100))["hits"]
        return {f"Hits@{k}": v for k, v in r.items()}
    return {"MRR": metrics.mrr(scores[pos], scores[neg])["MRR"]}


def fit_and_select(train, valid, test, *, eval_metric="auc", k_heuristic=0, k_pool_strategy="", hidden=256, epochs=10,
                   batch_size=32, lr=1e-3, seed=0, dropout=0.5):
    """The reference's epoch loop (sgrl_link_pred.py:1386-1428 with its Logger) on the fused trainer of
    `train_and_evaluate_fused`: after every epoch the valid and test splits are scored (`net.score`) and the chosen
    metric is computed from those device scores by one `metrics.LinkMetrics`, so no score comes to the host.
    eval_metric: 'auc' (keys AUC, AP), 'rocauc' (rocauc), 'hits' (Hits@20, Hits@50, Hits@100) or 'mrr' (MRR).
    train / valid / test: (rows, row_ptr, y) device tensors.  For 'mrr' a split holds num_pos positives and num_pos · M
    negatives, the negatives of positive i being negatives i·M .. i·M + M − 1 in the split's order.
    Returns dict(history {key: [(valid, test) per epoch]}, best_epoch {key: the first epoch of the highest valid
    value}, selected {key: test at that epoch}, trainer)."""
    from .metrics import LinkMetrics
    from .signnet import SIGNNetTrainer

    if eval_metric not in EVAL_METRICS:
        raise ValueError(f"eval_metric must be one of {EVAL_METRICS}, got {eval_metric!r}")
    if int(epochs) < 1:
        raise ValueError(f"need one epoch or more, got {epochs}")
    rows, row_ptr, y = train
    net = SIGNNetTrainer(rows.shape[1] * rows.shape[2], hidden, k_heuristic, k_pool_strategy, dropout, lr, seed=seed,
                         device=rows.device)
    rows, row_ptr, yf = net._store(rows, row_ptr, y)
    splits = _eval_splits(valid, test, eval_metric, net.engine.device)
    metrics = LinkMetrics(net.engine.device)
    history = {}
    try:
        for _ in range(epochs):
            net._epoch(rows, row_ptr, yf, batch_size)
            res = [_epoch_metric(metrics, eval_metric, net.score(s[0], s[1]), sp)
                   for s, sp in zip((valid, test), splits)]
            for key in res[0]:
                history.setdefault(key, []).append((res[0][key], res[1][key]))
    finally:
        metrics.close()
    return dict(_selected(history), trainer=net)


def _eval_splits(valid, test, eval_metric, device):
    """[(labels, positive ids, negative ids) on the device] of the valid and the test split, read once before the
    epoch loop; the ids only for 'mrr'."""
    splits = []
    for _, _, y_s in (valid, test):
        y_s = torch.as_tensor(y_s).to(device)
        pos = neg = None
        if eval_metric == "mrr":
            pos, neg = torch.nonzero(y_s == 1).view(-1), torch.nonzero(y_s == 0).view(-1)
            if pos.numel() == 0 or neg.numel() == 0 or neg.numel() % pos.numel():
                raise ValueError(f"mrr needs M negatives per positive, got {neg.numel()} for {pos.numel()}")
        splits.append((y_s, pos, neg))
    return splits


def _selected(history):
    """history {key: [(valid, test) per epoch]} -> dict(history, best_epoch, selected) as `fit_and_select` returns."""
    best = {key: max(range(len(h)), key=lambda e: (h[e][0], -e)) for key, h in history.items()}
    return {"history": history, "best_epoch": best, "selected": {key: history[key][e][1] for key, e in best.items()}}


def run_statistics(history_per_run):
    """What the reference's Logger prints for all runs (utils.py:769-792), as data.  history_per_run: one history
    {key: [(valid, test) per epoch]} per run, every run with the same keys and epochs.  Per key, values × 100 in fp32
    as the Logger holds them:
      per_run        [{"highest_valid", "best_epoch" (the first epoch of the highest valid), "highest_test" (the test
                     value at that epoch)}]
      highest_valid  {"mean", "std"} of the runs' highest valid (std unbiased, as torch's: NaN for one run)
      highest_test   {"mean", "std"} of the runs' test at their best epoch
      average_test   {"mean", "std"} of test over all epochs × runs
      highest_test_5 the Logger's "(Precision of 5)" line: "mean ± std" with five decimals"""
    runs = list(history_per_run)
    if not runs:
        raise ValueError("need the history of one run or more")
    out = {}
    for key in runs[0]:
        for h in runs:
            if key not in h or len(h[key]) != len(runs[0][key]) or not len(h[key]):
                raise ValueError(f"every run needs {key!r} with the same number (one or more) of epochs")
        result = 100 * torch.tensor([[tuple(e) for e in h[key]] for h in runs])      # [runs, epochs, 2]
        at = result[:, :, 0].argmax(dim=1)                                          # the first of equal maxima
        valid = result[:, :, 0].max(dim=1).values
        test = result[torch.arange(len(runs)), at, 1]
        every = result[:, :, 1].reshape(-1)

        def ms(t):
            return {"mean": float(t.mean()), "std": float(t.std()) if t.numel() > 1 else float("nan")}

        out[key] = {"per_run": [{"highest_valid": float(v), "best_epoch": int(e), "highest_test": float(t)}
                                for v, e, t in zip(valid, at, test)],
                    "highest_valid": ms(valid), "highest_test": ms(test), "average_test": ms(every),
                    "highest_test_5": "{mean:.5f} ± {std:.5f}".format(**ms(test))}
    return out


def fit_and_select_runs(train, valid, test, *, runs=10, eval_metric="auc", k_heuristic=0, k_pool_strategy="",
                        hidden=256, epochs=10, batch_size=32, lr=1e-3, seed=0, dropout=0.5):
    """`fit_and_select` for the `runs` runs of a config (the reference's `for run in range(args.runs)`, sgrl_link_pred.py
    :1281), trained side by side by `signnet.SIGNNetRuns`: run r has seed `seed + r` and is bit-identical to
    `fit_and_select(..., seed=seed + r)`.  After every epoch every member scores valid and test.  Returns dict(runs
    [dict(history, best_epoch, selected) per run], statistics `run_statistics` of the histories, trainer the group)."""
    from .metrics import LinkMetrics
    from .signnet import SIGNNetRuns

    if eval_metric not in EVAL_METRICS:
        raise ValueError(f"eval_metric must be one of {EVAL_METRICS}, got {eval_metric!r}")
    if int(epochs) < 1:
        raise ValueError(f"need one epoch or more, got {epochs}")
    if int(runs) < 1:
        raise ValueError(f"need one run or more, got {runs}")
    rows, row_ptr, y = train
    group = SIGNNetRuns(rows.shape[1] * rows.shape[2], hidden, k_heuristic, k_pool_strategy, dropout, lr,
                        seeds=[int(seed) + r for r in range(int(runs))], device=rows.device)
    rows, row_ptr, yf = group.members[0]._store(rows, row_ptr, y)
    splits = _eval_splits(valid, test, eval_metric, group.engine.device)
    metrics = LinkMetrics(group.engine.device)
    histories = [{} for _ in group.members]
    try:
        for _ in range(epochs):
            group._epoch(rows, row_ptr, yf, batch_size)
            for net, history in zip(group.members, histories):
                res = [_epoch_metric(metrics, eval_metric, net.score(s[0], s[1]), sp)
                       for s, sp in zip((valid, test), splits)]
                for key in res[0]:
                    history.setdefault(key, []).append((res[0][key], res[1][key]))
    finally:
        metrics.close()
    return {"runs": [_selected(h) for h in histories], "statistics": run_statistics(histories), "trainer": group}


def train_and_evaluate_seal(train, test, *, model="DGCNN", hidden=32, num_layers=3, k=0.6, max_z=1000,
                            use_feature=False, use_edge_weight=False, dynamic_train=False, epochs=10,
                            batch_size=32, lr=1e-4, seed=0, dropout=0.5):
    """The SEAL baselines' loop (reference sgrl_link_pred.py: train :440-472, test :538-587) on the twins of
    s3grl_amd.seal_nn, shaped like `train_and_evaluate`: BCE with logits, Adam, shuffled batches (batches of
    fewer than two links are skipped: BatchNorm), AUC on the test split in batches of 1024 links.
    train / test: (subs, y) with subs the `SubgraphList` of a split's links (seal.enclosing_subgraphs) and y
    their labels, a device tensor [L].  Returns (test AUC, model)."""
    from .seal_nn import DGCNNTwin, GCNTwin

    if model not in ("DGCNN", "GCN"):
        raise NotImplementedError(f"model {model!r}: the SEAL twins are DGCNN and GCN")
    torch.manual_seed(seed)
    subs, y = train
    dev = y.device
    if model == "DGCNN":
        net = DGCNNTwin(hidden, num_layers, max_z, k, train_dataset=subs, dynamic_train=dynamic_train,
                        use_feature=use_feature).to(dev)
    else:
        net = GCNTwin(hidden, num_layers, max_z, train_dataset=subs, use_feature=use_feature,
                      dropout=dropout).to(dev)
    return _seal_loop(net, train, test, use_edge_weight=use_edge_weight, epochs=epochs, batch_size=batch_size, lr=lr)


def _seal_loop(net, train, test, *, use_edge_weight, epochs, batch_size, lr):
    """The loop shared by the SEAL entry points: Adam on `net`, shuffled batches of the train split, then the test
    split's AUC in batches of 1024 links.  Returns (test AUC, net)."""
    subs, y = train
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    L = len(subs)
    yf = y.float()
    for _ in range(epochs):
        net.train()
        perm = torch.randperm(L).numpy()
        for b in range(0, L, batch_size):
            ids = perm[b:b + batch_size]
            if ids.size < 2:          # BatchNorm needs two links
                continue
            batch = subs.batch(ids, use_edge_weight=use_edge_weight)
            loss = nn.functional.binary_cross_entropy_with_logits(net(batch).view(-1), yf[batch.link_ids_device])
            opt.zero_grad()
            loss.backward()
            opt.step()
    subs_t, y_t = test
    net.eval()
    out = []
    with torch.no_grad():
        for b in range(0, len(subs_t), 1024):
            batch = subs_t.batch(np.arange(b, min(b + 1024, len(subs_t))), use_edge_weight=use_edge_weight)
            out.append(net(batch).view(-1))
    return auc_score(torch.cat(out), y_t), net


def train_and_evaluate_seal_mpnn(train, test, *, model="SAGE", hidden=32, num_layers=3, max_z=1000,
                                 use_feature=False, jk=True, train_eps=False, epochs=10, batch_size=32, lr=1e-4,
                                 seed=0, dropout=0.5):
    """`train_and_evaluate_seal` for the message-passing SEAL models of s3grl_amd.mpnn: model "SAGE" (`SAGETwin`) or
    "GIN" (`GINTwin`, with jk and train_eps).  Same loop, arguments and return value: (test AUC, model)."""
    from .mpnn import GINTwin, SAGETwin

    if model not in ("SAGE", "GIN"):
        raise NotImplementedError(f"model {model!r}: the message-passing SEAL twins are SAGE and GIN")
    torch.manual_seed(seed)
    subs, y = train
    dev = y.device
    if model == "SAGE":
        net = SAGETwin(hidden, num_layers, max_z, train_dataset=subs, use_feature=use_feature, dropout=dropout).to(dev)
    else:
        net = GINTwin(hidden, num_layers, max_z, train_dataset=subs, use_feature=use_feature, dropout=dropout, jk=jk,
                      train_eps=train_eps).to(dev)
    return _seal_loop(net, train, test, use_edge_weight=False, epochs=epochs, batch_size=batch_size, lr=lr)
