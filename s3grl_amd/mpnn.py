"""Message passing on the raw edge list: PyG SAGEConv and GINConv and global_mean_pool, and on them the twins of the
reference's SEAL models `SAGE` (models.py:78-135) and `GIN` (models.py:225-298).  The graph work runs as HIP kernels
behind the C ABI (s3grl_nbr_aggregate, csrc/s3grl_propagate.hip; s3grl_segment_mean_forward / _backward,
csrc/s3grl_mpnn.hip); the aggregation's structure and operator live in `propagate`.

    subs = enclosing_subgraphs(link_index, A, x, y, num_hops, node_label="drnl")
    model = SAGETwin(32, 3, max_z=1000, train_dataset=subs).cuda()
    logits = model(subs.batch(link_ids))                      # [B, 1]

    g = NbrGraph(edge_index, num_nodes)                       # a whole graph (s3grl_amd.mpgnn)
    out = aggregate(h, g, "mean")

Unlike the GCN operator (`seal_nn.gcn_propagate`) the edge list is taken as it is: an (i, i) entry is an edge, a
duplicated arc counts twice, no loop is added and nothing is normalised per edge.
  * `aggregate(h, op, "sum", self_coef)` is  self_coef · h[i] + Σ_{j -> i} h[j];
  * `aggregate(h, op, "mean")` divides the sum by the in-degree; a node without in-arcs gets a zero row (PyG's
    scatter-mean clamps the count at 1).  The mean's scale 1 / max(indeg, 1) is a small torch expression
    evaluated once per split / graph, not a kernel.
  * The backward is the same kernel on the CSR grouped by source; for the mean the weight of an arc belongs to its
    destination, so the scale is then read per neighbour.
Layers aggregate on the narrower side of their first linear map (aggregation commutes with it).  Deterministic: two
runs give bit-identical outputs and gradients.  GPU only; no CPU fallback.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

from . import _native as N
from .engine import default_engine
from .pool import centre_pool
from .propagate import MODES, NbrGraph, NbrSplit, aggregate  # noqa: F401  (this module's API)
from .seal_nn import MLP, _check_unused, _in_channels, _node_input

_SEG_CHUNK = 2048          # kSegChunk of csrc/s3grl_mpnn.hip


class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, node_ptr, max_nodes):
        eng = default_engine(x.device)
        x = x.contiguous()
        G, W = node_ptr.numel() - 1, x.shape[1]
        out = torch.empty((G, W), dtype=torch.float32, device=x.device)
        chunks = max(-(-max_nodes // _SEG_CHUNK), 1)
        partial = torch.empty(G * chunks * W, dtype=torch.float32, device=x.device) if chunks > 1 else None
        N.check(N.lib().s3grl_segment_mean_forward(eng._ctx, N.ptr(x), N.ptr(node_ptr), G, W, max_nodes, N.ptr(partial),
                                                   N.ptr(out)), "s3grl_segment_mean_forward")
        ctx.node_ptr, ctx.max_nodes, ctx.rows = node_ptr, max_nodes, x.shape[0]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        eng = default_engine(grad_out.device)
        grad_out = grad_out.contiguous()
        G, W = grad_out.shape
        gx = torch.empty((ctx.rows, W), dtype=torch.float32, device=grad_out.device)
        N.check(N.lib().s3grl_segment_mean_backward(eng._ctx, N.ptr(ctx.node_ptr), G, W, ctx.max_nodes, N.ptr(grad_out),
                                                    N.ptr(gx)), "s3grl_segment_mean_backward")
        return gx, None, None


def segment_mean(x, node_ptr, max_nodes=None):
    """global_mean_pool: x fp32 [n, W] on the GPU, graph g = rows node_ptr[g] .. node_ptr[g+1] (int64 [G+1] on the
    GPU, node_ptr[0] = 0, node_ptr[G] = n).  Returns [G, W], a zero row for an empty graph; differentiable in x.
    max_nodes: the largest graph's size when the host knows it (else one device -> host read)."""
    if not x.is_cuda:
        raise RuntimeError("segment_mean runs on the MI355X only; there is no CPU fallback")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] < 1 or node_ptr.dtype != torch.int64 or \
            node_ptr.dim() != 1 or node_ptr.numel() < 1:
        raise ValueError("x must be float32 [n, W] and node_ptr int64 [G+1]")
    if max_nodes is None:
        max_nodes = int(node_ptr.diff().max()) if node_ptr.numel() > 1 else 0
    return _SegmentMean.apply(x, node_ptr.contiguous(), int(max_nodes))


def _lin(x, weight):
    return weight.t() if x is None else x @ weight.t()   # x = None: identity features, x @ W^T = W^T


class SAGEConv(nn.Module):
    """PyG 2.0.x SAGEConv(in, out) (mean aggregation, root_weight, bias): lin_l(mean_{j -> i} x_j) + lin_r(x_i), with
    parameters `lin_l.weight`, `lin_l.bias` and `lin_r.weight` (torch's Linear init), the keys of PyG's state_dict.
    forward(x, op): x [n, in] or None for identity features (n = in); op a batch or an `NbrGraph`."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.lin_l = nn.Linear(in_channels, out_channels, bias=True)
        self.lin_r = nn.Linear(in_channels, out_channels, bias=False)

    def forward(self, x, op):
        if x is None or self.in_channels > self.out_channels:     # the mean of the mapped rows: the narrower side
            both = _lin(x, torch.cat([self.lin_l.weight, self.lin_r.weight], 0))
            left, right = both[:, :self.out_channels], both[:, self.out_channels:]
            return aggregate(left.contiguous(), op, "mean") + self.lin_l.bias + right
        return self.lin_l(aggregate(x, op, "mean")) + self.lin_r(x)


class GINConv(nn.Module):
    """PyG GINConv(nn, eps, train_eps): nn((1 + eps) · x_i + Σ_{j -> i} x_j).  `eps` [1] is a buffer, or a parameter
    with train_eps; either way it is in the state_dict under `eps`.  With a fixed eps the kernel adds the self term;
    with train_eps it is added in torch so that autograd reaches eps."""

    def __init__(self, nn_module, eps=0.0, train_eps=False):
        super().__init__()
        self.nn = nn_module
        self.train_eps = bool(train_eps)
        if self.train_eps:
            self.eps = nn.Parameter(torch.tensor([float(eps)]))
        else:
            self.register_buffer("eps", torch.tensor([float(eps)]))
        self._eps_host = float(eps)

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._eps_host = None          # read again from the loaded buffer

    def _combine(self, h, op):
        if self.train_eps:
            return aggregate(h, op, "sum") + (1 + self.eps) * h
        if self._eps_host is None:
            self._eps_host = float(self.eps)
        return aggregate(h, op, "sum", self_coef=1.0 + self._eps_host)

    def forward(self, x, op):
        first = self.nn[0] if isinstance(self.nn, nn.Sequential) and len(self.nn) and \
            isinstance(self.nn[0], nn.Linear) else None
        if first is not None and (x is None or first.in_features > first.out_features):
            h = self._combine(_lin(x, first.weight).contiguous(), op)   # the sum of the mapped rows, then the bias
            if first.bias is not None:
                h = h + first.bias
            for layer in list(self.nn)[1:]:
                h = layer(h)
            return h
        if x is None:
            raise ValueError("x = None (identity features) needs an nn that starts with a Linear")
        return self.nn(self._combine(x, op))


def gin_mlp(in_channels, hidden_channels, batch_norm=True):
    """The reference's GIN body: Linear, ReLU, Linear, ReLU (, BatchNorm1d)."""
    layers = [nn.Linear(in_channels, hidden_channels), nn.ReLU(), nn.Linear(hidden_channels, hidden_channels),
              nn.ReLU()]
    if batch_norm:
        layers.append(nn.BatchNorm1d(hidden_channels))
    return nn.Sequential(*layers)


class SAGETwin(nn.Module):
    """Reference SAGE (models.py:78-135): z embedding (+ x), num_layers SAGE layers with ReLU and dropout between
    them, centre pooling x[src] · x[dst] (`pool.centre_pool`), MLP [hidden, hidden, 1]."""

    def __init__(self, hidden_channels, num_layers, max_z, train_dataset=None, use_feature=False,
                 node_embedding=None, dropout=0.5, dropedge=0.0):
        super().__init__()
        _check_unused(node_embedding, dropedge)
        self.use_feature = use_feature
        self.dropout = dropout
        self.z_embedding = nn.Embedding(max_z, hidden_channels)
        chans = [_in_channels(hidden_channels, use_feature, train_dataset)] + [hidden_channels] * num_layers
        self.convs = nn.ModuleList(SAGEConv(a, b) for a, b in zip(chans[:-1], chans[1:]))
        self.mlp = MLP([hidden_channels, hidden_channels, 1], dropout=dropout)

    def forward(self, batch):
        x = _node_input(self.z_embedding, self.use_feature, batch)
        for conv in self.convs[:-1]:
            x = F.dropout(F.relu(conv(x, batch)), p=self.dropout, training=self.training)
        x = self.convs[-1](x, batch)
        return self.mlp(centre_pool(x, batch.node_ptr))


class GINTwin(nn.Module):
    """Reference GIN (models.py:225-298): z embedding (+ x), `conv1` and num_layers - 1 `convs`, each a GINConv around
    Linear, ReLU, Linear, ReLU, BatchNorm1d; the layer outputs concatenated (jk) or the last one, mean-pooled per
    subgraph (`segment_mean`), MLP [num_layers · hidden or hidden, hidden, 1] with dropout 0.5.  As in the reference,
    `dropout` is stored and not applied between the layers."""

    def __init__(self, hidden_channels, num_layers, max_z, train_dataset=None, use_feature=False,
                 node_embedding=None, dropout=0.5, jk=True, train_eps=False, dropedge=0.0):
        super().__init__()
        _check_unused(node_embedding, dropedge)
        self.use_feature = use_feature
        self.jk = jk
        self.dropout = dropout
        self.z_embedding = nn.Embedding(max_z, hidden_channels)
        first = _in_channels(hidden_channels, use_feature, train_dataset)
        self.conv1 = GINConv(gin_mlp(first, hidden_channels), train_eps=train_eps)
        self.convs = nn.ModuleList(GINConv(gin_mlp(hidden_channels, hidden_channels), train_eps=train_eps)
                                   for _ in range(num_layers - 1))
        self.mlp = MLP([num_layers * hidden_channels if jk else hidden_channels, hidden_channels, 1], dropout=0.5)

    def forward(self, batch):
        x = self.conv1(_node_input(self.z_embedding, self.use_feature, batch), batch)
        xs = [x]
        for conv in self.convs:
            x = conv(x, batch)
            xs.append(x)
        x = torch.cat(xs, dim=1) if self.jk else xs[-1]
        return self.mlp(segment_mean(x, batch.node_ptr, batch.max_nodes))
