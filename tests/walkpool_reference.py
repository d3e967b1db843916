"""Test infrastructure: a dense restatement of WalkPool in torch, written from the math, fp64 or fp32,
differentiable by torch autograd.  Per subgraph it builds the dense P+ and P- from the arcs, takes matrix powers and
forms the features; `DenseLinkPred` is the whole model with the GCN as the dense D^-1/2 (A+ + I) D^-1/2.

A subgraph is (n, src, dst): local nodes 0 .. n-1, the candidate link (0, 1), E- as arcs src -> dst (both directions of
an undirected edge listed).  PyG and torch_scatter are not installed here, so nothing below could be checked by running
the reference; tests/test_walkpool_host.py pins it with hand-derived answers instead."""
import math

import torch
from torch import nn
from torch.nn import functional as F


def plus_arcs(src, dst):
    """E+ = E- with 0 -> 1 and 1 -> 0 appended, and the mask that is False on those two."""
    src, dst = torch.as_tensor(src, dtype=torch.long), torch.as_tensor(dst, dtype=torch.long)
    mask = torch.ones(src.numel() + 2, dtype=torch.bool)
    mask[-2:] = False
    return torch.cat([src, torch.tensor([0, 1])]), torch.cat([dst, torch.tensor([1, 0])]), mask


def attention_dense(q, k, n, src, dst):
    """q, k [n, heads, hidden] of one subgraph -> (P+ [heads, n, n], P- [heads, n, n], omega [heads], w [e+, heads]);
    P[h, c, r] is the weight of the arc r -> c."""
    s, d, mask = plus_arcs(src, dst)
    hidden = q.shape[-1]
    w = (q[s] * k[d]).sum(-1) / math.sqrt(hidden)                    # [e+, heads]
    heads = w.shape[1]
    dense = torch.full((heads, n, n), -math.inf, dtype=w.dtype)
    dense = dense.index_put((torch.arange(heads)[None, :].expand_as(w), d[:, None].expand_as(w),
                             s[:, None].expand_as(w)), w)
    arc = torch.isfinite(dense)
    mx = dense.detach().max(dim=-1, keepdim=True).values             # over E+; a constant, as in PyG's softmax
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    ex = torch.where(arc, torch.exp(torch.where(arc, dense, torch.zeros_like(dense)) - mx), torch.zeros_like(dense))
    minus = torch.ones((n, n), dtype=torch.bool)
    minus[0, 1] = minus[1, 0] = False
    exm = ex * minus
    Pp = ex / (ex.sum(-1, keepdim=True) + 1e-16)
    Pm = exm / (exm.sum(-1, keepdim=True) + 1e-16)
    omega = torch.sigmoid(w[~mask]).sum(0)
    return Pp, Pm, omega, w


def walk_features(Pp, Pm, walk_len):
    """[heads, walk_len, 5]: graphlevel, nodelevel_p, nodelevel_m, linklevel_p, linklevel_m of tau = t + 2; and
    the two traces [heads, walk_len, 2] (the magnitude the graphlevel bound refers to)."""
    rows, traces = [], []
    Xp, Xm = Pp, Pm
    for _ in range(walk_len):
        Xp, Xm = Xp @ Pp, Xm @ Pm
        trp, trm = Xp.diagonal(dim1=-2, dim2=-1).sum(-1), Xm.diagonal(dim1=-2, dim2=-1).sum(-1)
        rows.append(torch.stack([trp - trm, Xp[:, 0, 0] + Xp[:, 1, 1], Xm[:, 0, 0] + Xm[:, 1, 1],
                                 Xp[:, 0, 1] + Xp[:, 1, 0], Xm[:, 0, 1] + Xm[:, 1, 0]], dim=-1))
        traces.append(torch.stack([trp, trm], dim=-1))
    return torch.stack(rows, dim=1), torch.stack(traces, dim=1)


def feature_row(walks, omega):
    """[heads·(5·walk_len + 1)]: [graphlevel | omega | nodelevel_p | nodelevel_m | linklevel_p | linklevel_m], each
    walk group indexed head·walk_len + t."""
    g = [walks[..., c].reshape(-1) for c in range(5)]
    return torch.cat([g[0], omega, g[1], g[2], g[3], g[4]])


def weights_to_dense(w_arcs, n, src, dst):
    """[heads, n, n] with P[h, dst, src] = w_arcs[e, h] of given per-arc weights (arcs src -> dst)."""
    heads = w_arcs.shape[1]
    P = torch.zeros((heads, n, n), dtype=w_arcs.dtype)
    return P.index_put((torch.arange(heads)[None, :].expand_as(w_arcs), dst[:, None].expand_as(w_arcs),
                        src[:, None].expand_as(w_arcs)), w_arcs)


def gcn_dense(n, src, dst, dtype):
    s, d, _ = plus_arcs(src, dst)
    A = torch.zeros((n, n), dtype=dtype)
    A[d, s] = 1.0
    A = A + torch.eye(n, dtype=dtype)
    dinv = A.sum(1).pow(-0.5)
    return dinv[:, None] * A * dinv[None, :]


class _Conv(nn.Module):
    def __init__(self, a, b):
        super().__init__()
        self.lin = nn.Linear(a, b, bias=False)
        self.bias = nn.Parameter(torch.zeros(b))


class _Wp(nn.Module):
    def __init__(self, a, hid, heads):
        super().__init__()
        self.lin_key1, self.lin_query1 = nn.Linear(a, hid), nn.Linear(a, hid)
        self.lin_key2, self.lin_query2 = nn.Linear(hid, heads * hid), nn.Linear(hid, heads * hid)


class _Mlp(nn.Module):
    def __init__(self, L):
        super().__init__()
        self.nn = nn.BatchNorm1d(L)
        self.linear1, self.linear2 = nn.Linear(L, 20 * L), nn.Linear(20 * L, 20 * L)
        self.linear3, self.linear4, self.linear5 = nn.Linear(20 * L, 10 * L), nn.Linear(10 * L, L), nn.Linear(L, 1)


class DenseLinkPred(nn.Module):
    """The whole model on dense matrices, dropout off; the parameter names of the twin, so its state_dict loads.
    forward(graphs, xs, zs): graphs a list of (n, src, dst), xs / zs the node features and labels per graph."""

    def __init__(self, in_channels, hidden, heads, walk_len, drnl=False, z_max=100, MSE=True):
        super().__init__()
        self.hidden, self.heads, self.walk_len, self.drnl, self.MSE = hidden, heads, walk_len, drnl, MSE
        if drnl:
            self.z_embedding = nn.Embedding(z_max, hidden)
        self.conv1, self.conv2 = _Conv(in_channels, hidden), _Conv(hidden, hidden)
        self.wp = _Wp(in_channels + 2 * hidden, hidden, heads)
        self.classifier = _Mlp(heads * (5 * walk_len + 1))

    def features(self, graphs, xs, zs=None):
        rows = []
        for g, (n, src, dst) in enumerate(graphs):
            x = xs[g]
            if self.drnl:
                x = torch.cat([x, self.z_embedding(zs[g])], dim=1)
            A = gcn_dense(n, src, dst, x.dtype)
            h1 = A @ self.conv1.lin(x) + self.conv1.bias
            h2 = A @ self.conv2.lin(h1.relu()) + self.conv2.bias
            xo = torch.cat([x, h1, h2], dim=1)
            q = self.wp.lin_key2(F.leaky_relu(self.wp.lin_key1(xo), 0.2)).view(n, self.heads, self.hidden)
            k = self.wp.lin_query2(F.leaky_relu(self.wp.lin_query1(xo), 0.2)).view(n, self.heads, self.hidden)
            Pp, Pm, omega, _ = attention_dense(q, k, n, src, dst)
            rows.append(feature_row(walk_features(Pp, Pm, self.walk_len)[0], omega))
        return torch.stack(rows)

    def forward(self, graphs, xs, zs=None):
        c = self.classifier
        x = c.nn(self.features(graphs, xs, zs))
        for lin in (c.linear1, c.linear2, c.linear3, c.linear4):
            x = F.relu(lin(x))
        x = c.linear5(x)
        return torch.sigmoid(x) if self.MSE else x
