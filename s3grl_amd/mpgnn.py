"""The message-passing rows of the reference's Table 2 (baselines/gnn_link_pred.py `Net` and `train_gnn`,
run_helpers/run_mpgnns.py): a three-layer whole-graph GCN, SAGE or GIN encoder, PyG's sparse negative sampling, an
inner-product decoder and BCE with logits.

    results = run_mpgnn(split, "SAGE")                        # {'AUC': (val, test), 'AP': (val, test)}

The graph work runs as HIP kernels: GCN through `gae.GcnGraph.propagate` (s3grl_gcn_propagate), SAGE and GIN through
`mpnn.aggregate` on an `mpnn.NbrGraph` (s3grl_nbr_aggregate), negatives and the decoder through s3grl_gae_*.  Same
model and training as PyG 2.0.x, as `train_gnn` runs them:
  * GCN: GCNConv (glorot linear, zero bias); SAGE: SAGEConv (mean); GIN: GINConv(Linear, ReLU, Linear, ReLU), eps
    fixed at 0, no BatchNorm; SAGE's and GIN's linears with torch's Linear init.  relu and dropout follow the first
    two layers only.  x = None is the identity matrix: x @ W^T is W^T, no N x N product.
  * one Adam step per epoch on the whole graph; as many negatives as train positives from
    negative_sampling(edge_index, N) every epoch; one BCEWithLogitsLoss mean over positives then negatives.
  * every eval_steps epochs val / test AUC and AP of sigmoid(z_u·z_v) in eval mode; the result is the test value at
    the FIRST epoch of maximal val value.
Parameter init comes from a torch generator seeded with `seed`, the negatives from the engine's counter-based
generator keyed by (seed, epoch): PyG's distributions, not its random streams.  GPU only; no CPU fallback.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.nn import functional as F

from . import gae
from .mpnn import GINConv, NbrGraph, SAGEConv, gin_mlp

LAYERS = ("GCN", "SAGE", "GIN")


def _linear_init(lin, gen):
    """torch.nn.Linear's default init (kaiming_uniform with a = sqrt(5): U(-1/sqrt(in), 1/sqrt(in)) for the weight and
    the bias), drawn from `gen`."""
    bound = 1.0 / math.sqrt(lin.in_features)
    with torch.no_grad():
        for p in (lin.weight, lin.bias):
            if p is not None:
                p.copy_(torch.rand(p.shape, generator=gen, dtype=torch.float64).mul_(2 * bound).sub_(bound).float())


class _GCNLayer(gae.GCNConvParams):
    def forward(self, x, graph):
        return graph.propagate(gae._lin(x, self.lin.weight), self.bias)


class NetTwin(nn.Module):
    """Reference gnn_link_pred.Net(in_channels, hidden_channels, layer): conv1, conv2, conv3 of GCN, SAGE or GIN
    layers with PyG's state_dict keys.  `graph` is `make_graph`'s operator for the layer kind."""

    def __init__(self, in_channels, hidden_channels, layer="GCN", *, seed=0):
        super().__init__()
        if layer not in LAYERS:
            raise NotImplementedError(f"Layer {layer} not supported")
        self.layer = layer
        gen = torch.Generator().manual_seed(int(seed))
        chans = [int(in_channels), int(hidden_channels), int(hidden_channels), int(hidden_channels)]
        for i, (a, b) in enumerate(zip(chans[:-1], chans[1:]), start=1):
            if layer == "GCN":
                conv = _GCNLayer(a, b, gen)
            elif layer == "SAGE":
                conv = SAGEConv(a, b)
                _linear_init(conv.lin_l, gen)
                _linear_init(conv.lin_r, gen)
            else:
                conv = GINConv(gin_mlp(a, b, batch_norm=False), train_eps=False)
                _linear_init(conv.nn[0], gen)
                _linear_init(conv.nn[2], gen)
            setattr(self, f"conv{i}", conv)

    def make_graph(self, edge_index, num_nodes, device=None):
        """The whole-graph operator this layer kind runs on."""
        return (gae.GcnGraph if self.layer == "GCN" else NbrGraph)(edge_index, num_nodes, device)

    def encode(self, x, graph, dropout):
        """x fp32 [N, in] or None for identity features; relu and dropout after the first two layers only."""
        x = F.dropout(self.conv1(x, graph).relu(), p=dropout, training=self.training)
        x = F.dropout(self.conv2(x, graph).relu(), p=dropout, training=self.training)
        return self.conv3(x, graph)

    def decode(self, z, edge_label_index):
        """z_u · z_v of every pair ([2, L] or a `gae.PairList`): logits fp32 [L]."""
        return gae.inner_product_decode(z, edge_label_index)


def train(edge_index, x, split_lists, model, *, hidden=32, lr=0.01, epochs=50, eval_steps=1, dropout=0.5, seed=0,
          num_nodes=None, device=None, on_epoch=None):
    """The loop of train_gnn.  edge_index [2, E]: the message-passing graph; split_lists = [train_pos, test_pos,
    test_neg, val_pos, val_neg] ([2, L] each); x [N, F] or None for eye(N) (then num_nodes is needed).  Returns
    (per-eval results {'AUC': [(val, test)], 'AP': [...]}, the model, per-epoch losses as fp32 device tensor)."""
    if model not in LAYERS:
        raise NotImplementedError(f"Layer {model} not supported")
    ei = gae._as_pairs(edge_index)
    if x is not None:
        x = torch.as_tensor(x)
        if x.dim() != 2:
            raise ValueError("x must be [N, F]")
        n = x.shape[0] if num_nodes is None else int(num_nodes)
        if x.shape[0] != n:
            raise ValueError(f"x has {x.shape[0]} rows, the graph {n} nodes")
    else:
        if num_nodes is None:
            raise ValueError("x = None (identity features) needs num_nodes")
        n = int(num_nodes)
    if len(split_lists) != 5:
        raise ValueError("split_lists must be [train_pos, test_pos, test_neg, val_pos, val_neg]")
    lists = [gae.check_ids(t, n) for t in split_lists]
    gae.check_ids(ei, n)
    epochs, eval_steps = int(epochs), int(eval_steps)
    if epochs < 0 or eval_steps < 1 or not lr > 0 or not 0 <= dropout < 1:
        raise ValueError("need epochs >= 0, eval_steps >= 1, lr > 0 and dropout in [0, 1)")
    dev = gae.check_device(device)

    eng = gae._engine(dev)
    dev = eng.device
    torch.manual_seed(seed)                      # the dropout masks
    xs = x.to(device=dev, dtype=torch.float32).contiguous() if x is not None else None
    net = NetTwin(n if x is None else x.shape[1], hidden, model, seed=seed).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=lr)
    graph = net.make_graph(ei, n, dev)
    pos = gae.PairList(ei, n, dev)               # what the negatives avoid
    pos.keys()
    train_pos, test_pos, test_neg, val_pos, val_neg = (gae.PairList(t, n, dev) for t in lists)
    eval_lists = {"val": (val_pos, val_neg), "test": (test_pos, test_neg)}
    results = {"AUC": [], "AP": []}
    losses = torch.empty(epochs, dtype=torch.float32, device=dev)
    P = len(train_pos)
    for epoch in range(1, epochs + 1):
        net.train()
        opt.zero_grad(set_to_none=True)
        z = net.encode(xs, graph, dropout)
        neg = gae._sample(pos, P, seed, epoch)
        pairs = gae.PairList._wrap(torch.cat([train_pos.src, neg.src]), torch.cat([train_pos.dst, neg.dst]), n, eng)
        label = torch.cat([torch.ones(P, device=dev), torch.zeros(len(neg), device=dev)])
        loss = F.binary_cross_entropy_with_logits(net.decode(z, pairs), label)
        loss.backward()
        opt.step()
        losses[epoch - 1] = loss.detach()
        if on_epoch is not None:
            on_epoch(epoch)
        if epoch % eval_steps == 0:
            net.eval()
            with torch.no_grad():
                res = gae._evaluate(net.encode(xs, graph, dropout).detach(), eval_lists)
            for key in results:
                results[key].append(res[key])
    return results, net, losses


def split_lists(split):
    """[train_pos, test_pos, test_neg, val_pos, val_neg] of a `workloads.Split`."""
    return [split.links["train"][0], split.links["test"][0], split.links["test"][1], split.links["valid"][0],
            split.links["valid"][1]]


def run_mpgnn(split, model, x=None, *, epochs=50, hidden=32, lr=0.01, dropout=0.5, seed=1, device=None):
    """One Table 2 message-passing row from a `workloads.Split` (run_helpers/run_mpgnns.py; x = None is eye(N)):
    {'AUC': (best val, test at it), 'AP': (...)}, each chosen at the first epoch of its own maximal val value, as
    fractions (like gae.run_gae)."""
    results, _, _ = train(split.edge_index(), x, split_lists(split), model, hidden=hidden, lr=lr, epochs=epochs,
                          eval_steps=1, dropout=dropout, seed=seed, num_nodes=split.num_nodes, device=device)
    if not results["AUC"]:
        raise ValueError("epochs must be >= 1")
    return {k: tuple(float(v) for v in gae.best_at_first_max(r)) for k, r in results.items()}
