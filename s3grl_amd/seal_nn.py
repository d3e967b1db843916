"""The SEAL baselines' models on labelled enclosing subgraphs: twins of reference `models.DGCNN` (models.py:139-222)
and `models.GCN` (models.py:12-76) whose graph operators are HIP kernels behind the C ABI
(s3grl_gcn_norm / _gcn_propagate, csrc/s3grl_propagate.hip; s3grl_sort_pool_forward / _backward,
csrc/s3grl_seal_nn.hip).

    subs = enclosing_subgraphs(link_index, A, x, y, num_hops, node_label="drnl")
    model = DGCNNTwin(32, 3, max_z=1000, k=0.6, train_dataset=subs).cuda()
    logits = model(subs.batch(link_ids))                      # [B, 1]

The reference builds them on PyG's GCNConv and global_sort_pool; here
  * `gcn_propagate` is GCNConv's message passing after its linear (gcn_norm with add_remaining_self_loops,
    flow source -> target).  Its structure (both edge orders, per-node pointers, dinv and the coefficients) is
    built once per split (`propagate.GcnSplit`) and reused by every batch, layer and epoch.
  * `sort_pool` is global_sort_pool, with ties broken by ascending node position and -0.0 == +0.0.
Both are deterministic: two runs give bit-identical outputs and gradients.  GPU only; no CPU fallback.
"""
from __future__ import annotations

import math

import torch
from torch import nn
from torch.nn import functional as F

from . import _native as N
from .engine import default_engine
from .pool import centre_pool
from .propagate import GcnSplit, gcn_propagate  # noqa: F401  (GCNConv calls gcn_propagate as this module's name)

_DEFAULT_SORT_LDS = 64 << 10
_MAX_SORT_LDS = 159 << 10


def _sort_lds_bytes(lds_budget):
    return min(int(lds_budget), _MAX_SORT_LDS) if lds_budget > 0 else _DEFAULT_SORT_LDS


class _SortPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, node_ptr, k, max_nodes, lds_budget):
        eng = default_engine(x.device)
        x = N.aligned16(x.contiguous())      # float4 row copies when D % 4 == 0
        G, D = node_ptr.numel() - 1, x.shape[1]
        out = torch.empty((G, k * D), dtype=torch.float32, device=x.device)
        index = torch.empty((G, k), dtype=torch.int32, device=x.device)
        P = 1 << max(int(max_nodes) - 1, 0).bit_length()
        ws = None
        if P * 8 > _sort_lds_bytes(lds_budget):
            ws = torch.empty(max(2 * x.shape[0], 1), dtype=torch.int64, device=x.device)
        N.check(N.lib().s3grl_sort_pool_forward(eng._ctx, N.ptr(x), N.ptr(node_ptr), G, D, k, int(max_nodes),
                                                int(lds_budget), N.ptr(ws), N.ptr(out), N.ptr(index)),
                "s3grl_sort_pool_forward")
        ctx.save_for_backward(index)
        ctx.shape = (x.shape[0], D, k)
        ctx.mark_non_differentiable(index)
        return out, index

    @staticmethod
    def backward(ctx, grad_out, _grad_index):
        (index,) = ctx.saved_tensors
        R, D, k = ctx.shape
        eng = default_engine(grad_out.device)
        grad_out = N.aligned16(grad_out.contiguous())
        gx = torch.empty((R, D), dtype=torch.float32, device=grad_out.device)
        N.check(N.lib().s3grl_sort_pool_backward(eng._ctx, index.shape[0], D, k, N.ptr(index), N.ptr(grad_out), R,
                                                 N.ptr(gx)), "s3grl_sort_pool_backward")
        return gx, None, None, None, None


def sort_pool(x, node_ptr, k, max_nodes=None, lds_budget=0, return_index=False):
    """global_sort_pool: x fp32 [n, D] on the GPU, graph g = rows node_ptr[g] .. node_ptr[g+1] (int64 [G+1] on
    the GPU).  Returns [G, k·D]: every graph's rows by x[:, -1] descending (ties by ascending row, -0.0 == +0.0),
    the first k, zero rows past its size.  max_nodes: the largest graph's size when the host knows it (else
    one device -> host read); lds_budget: bytes of LDS a graph's sort may use (0 = 64 KiB; 1 sorts in HBM)."""
    if not x.is_cuda:
        raise RuntimeError("sort_pool runs on the MI355X only; there is no CPU fallback")
    if x.dtype != torch.float32 or x.dim() != 2 or node_ptr.dtype != torch.int64:
        raise ValueError("x must be float32 [n, D] and node_ptr int64 [G+1]")
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError("k must be an integer >= 1")
    if int(lds_budget) < 0:
        raise ValueError("lds_budget must be >= 0")
    if x.shape[0] >= 2**31:
        raise ValueError("sort_pool indexes rows with int32: at most 2^31 - 1 rows")
    if max_nodes is None:
        max_nodes = int(node_ptr.diff().max()) if node_ptr.numel() > 1 else 0
    out, index = _SortPool.apply(x, node_ptr, int(k), int(max_nodes), int(lds_budget))
    return (out, index) if return_index else out


def sortpool_k(node_counts, k=0.6, dynamic_train=False):
    """The reference's k (models.py:144-155): k <= 1 is a percentile of the training graphs' node counts
    (the first 1000 with dynamic_train), at least 10; k > 1 is used as it is; 30 without training graphs."""
    if k > 1:
        return int(k)
    if node_counts is None:
        return 30
    counts = [int(c) for c in node_counts]
    if dynamic_train:
        counts = counts[:1000]
    if not counts:
        raise ValueError("sortpool_k needs at least one training graph")
    counts = sorted(counts)
    return int(max(10, counts[int(math.ceil(k * len(counts))) - 1]))


class GCNConv(nn.Module):
    """PyG GCNConv(in, out) (improved=False, add_self_loops, normalize, bias): parameters `lin.weight`
    [out, in] (glorot, no bias in the linear) and `bias` [out] (zeros), the keys of PyG's state_dict."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        self.bias = nn.Parameter(torch.zeros(out_channels))
        nn.init.xavier_uniform_(self.lin.weight)

    def forward(self, x, batch):
        return gcn_propagate(self.lin(x), batch, self.bias)


class MLP(nn.Module):
    """PyG MLP(channels, dropout, batch_norm=True): Linear -> BatchNorm -> ReLU -> Dropout per hidden layer,
    a plain Linear last (state_dict keys lins.* / norms.*)."""

    def __init__(self, channels, dropout=0.5):
        super().__init__()
        self.lins = nn.ModuleList(nn.Linear(a, b) for a, b in zip(channels[:-1], channels[1:]))
        self.norms = nn.ModuleList(nn.BatchNorm1d(c) for c in channels[1:-1])
        self.dropout = dropout

    def forward(self, x):
        for lin, norm in zip(self.lins[:-1], self.norms):
            x = F.dropout(F.relu(norm(lin(x))), p=self.dropout, training=self.training)
        return self.lins[-1](x)


def _check_unused(node_embedding, dropedge):
    if node_embedding is not None:
        raise NotImplementedError("node_embedding: no paper config uses it")
    if dropedge:
        raise NotImplementedError("dropedge > 0: no paper config uses it")


def _in_channels(hidden, use_feature, train_dataset):
    if not use_feature:
        return hidden
    if train_dataset is None or getattr(train_dataset, "x", None) is None:
        raise ValueError("use_feature needs a train_dataset with node features")
    return hidden + int(train_dataset.x.shape[1])


def _node_input(z_embedding, use_feature, batch):
    z_emb = z_embedding(batch.z)
    if z_emb.dim() == 3:                 # de / de+: one embedding per label column, summed
        z_emb = z_emb.sum(dim=1)
    if use_feature and batch.x is not None:
        return torch.cat([z_emb, batch.x.to(torch.float)], 1)
    return z_emb


class DGCNNTwin(nn.Module):
    """Reference DGCNN (models.py:139-222) with GCNConv layers: z embedding (+ x), num_layers GCN layers of
    width hidden_channels and one of width 1, each followed by tanh, concatenated (D = hidden·num_layers + 1);
    sort pool with k; Conv1d(1, 16, D, stride D), ReLU, MaxPool1d(2, 2), Conv1d(16, 32, 5), ReLU; MLP
    [dense_dim, 128, 1].  `train_dataset`: the training `SubgraphList` (node counts for k, feature width)."""

    def __init__(self, hidden_channels, num_layers, max_z, k=0.6, train_dataset=None, dynamic_train=False,
                 use_feature=False, node_embedding=None, dropedge=0.0):
        super().__init__()
        _check_unused(node_embedding, dropedge)
        counts = train_dataset.node_counts() if train_dataset is not None else None
        self.k = sortpool_k(counts, k, dynamic_train)
        self.use_feature = use_feature
        self.z_embedding = nn.Embedding(max_z, hidden_channels)
        chans = [_in_channels(hidden_channels, use_feature, train_dataset)] + [hidden_channels] * num_layers + [1]
        self.convs = nn.ModuleList(GCNConv(a, b) for a, b in zip(chans[:-1], chans[1:]))
        D = hidden_channels * num_layers + 1
        self.conv1 = nn.Conv1d(1, 16, D, D)
        self.maxpool1d = nn.MaxPool1d(2, 2)
        self.conv2 = nn.Conv1d(16, 32, 5, 1)
        dense_dim = (int((self.k - 2) / 2 + 1) - 5 + 1) * 32
        if dense_dim <= 0:
            raise ValueError(f"k = {self.k} leaves no input for the MLP")
        self.mlp = MLP([dense_dim, 128, 1], dropout=0.5)

    def forward(self, batch):
        xs = [_node_input(self.z_embedding, self.use_feature, batch)]
        for conv in self.convs:
            xs.append(torch.tanh(conv(xs[-1], batch)))
        x = torch.cat(xs[1:], dim=-1)
        B, D, k = batch.num_graphs, x.shape[1], self.k
        x = sort_pool(x, batch.node_ptr, k, batch.max_nodes)                        # [B, k·D]
        # Conv1d(1, 16, D, stride D) is one linear map of every pooled row
        x = F.linear(x.view(B * k, D), self.conv1.weight.view(16, D), self.conv1.bias)
        x = F.relu(x.view(B, k, 16).transpose(1, 2))                               # [B, 16, k]
        x = self.maxpool1d(x)
        # Conv1d(16, 32, 5) as one matrix product over the unfolded windows
        L = x.shape[2] - 4
        x = x.unfold(2, 5, 1).permute(0, 2, 1, 3).reshape(B * L, 80)
        x = F.linear(x, self.conv2.weight.view(32, 80), self.conv2.bias)
        x = F.relu(x.view(B, L, 32).transpose(1, 2))                               # [B, 32, k//2 - 4]
        return self.mlp(x.reshape(B, -1))


class GCNTwin(nn.Module):
    """Reference GCN (models.py:12-76): z embedding (+ x), num_layers GCN layers with ReLU and dropout between
    them, centre pooling x[src] · x[dst] (`pool.centre_pool`), MLP [hidden, hidden, 1]."""

    def __init__(self, hidden_channels, num_layers, max_z, train_dataset=None, use_feature=False,
                 node_embedding=None, dropout=0.5, dropedge=0.0):
        super().__init__()
        _check_unused(node_embedding, dropedge)
        self.use_feature = use_feature
        self.dropout = dropout
        self.z_embedding = nn.Embedding(max_z, hidden_channels)
        chans = [_in_channels(hidden_channels, use_feature, train_dataset)] + [hidden_channels] * num_layers
        self.convs = nn.ModuleList(GCNConv(a, b) for a, b in zip(chans[:-1], chans[1:]))
        self.mlp = MLP([hidden_channels, hidden_channels, 1], dropout=dropout)

    def forward(self, batch):
        x = _node_input(self.z_embedding, self.use_feature, batch)
        for conv in self.convs[:-1]:
            x = F.dropout(F.relu(conv(x, batch)), p=self.dropout, training=self.training)
        x = self.convs[-1](x, batch)
        return self.mlp(centre_pool(x, batch.node_ptr))
