"""Neighbour aggregation over a split of subgraphs or over a whole graph: the structure the kernel of
csrc/s3grl_propagate.hip reads, built once, and the two differentiable operators on it (s3grl_gcn_norm /
_gcn_propagate / _nbr_aggregate behind the C ABI).

One structure serves both: the arcs src -> dst over n nodes as a CSR by destination (forward) and one by source
(backward, the transposed operator), the neighbour as a position inside its own subgraph, and `loc`, every node's
position in its subgraph.  A whole graph is the split of one subgraph holding every node: rows = loc = arange(N), nbr
= the global id.  The two operator kinds differ in what they make of the arcs:
  * GCN (`GcnSplit`, `GcnGraph`, `gcn_propagate`): GCNConv's message passing after its linear.  Input (i, i) entries
    are replaced by one loop per node (add_remaining_self_loops), and every arc carries coef = dinv[src] · w ·
    dinv[dst] (gcn_norm).
  * raw (`NbrSplit`, `NbrGraph`, `aggregate`): SAGEConv's mean and GINConv's sum.  The edge list is taken as it is:
    an (i, i) entry is an edge, a duplicated arc counts twice, and the mean's scale = 1 / max(indeg, 1) is per node.
    The backward of the mean reads the scale per neighbour: the weight of an arc belongs to its destination.
  * GIC (`GicGraph`, `gic_arcs`): the operator D·(A + I)ᵀ·D of Graph InfoClust's CalGIC, on gcn_propagate's kernel
    with its own coefficients.  Duplicated arcs add up, an input (i, i) entry is kept and the identity is added to it,
    and D = rowsum(A + I)^-1/2 by SOURCE row.
Deterministic: two runs give bit-identical outputs and gradients.  GPU only; no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from .engine import default_engine

MODES = ("sum", "mean")


def _as_pairs(edge_index):
    ei = edge_index if isinstance(edge_index, torch.Tensor) else torch.as_tensor(np.asarray(edge_index))
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(ei.shape)}")
    if ei.dtype.is_floating_point or ei.dtype == torch.bool:
        raise ValueError(f"edge_index must hold integer node ids, got {ei.dtype}")
    return ei


def check_ids(edge_index, num_nodes):
    """ValueError unless every id of edge_index [2, E] is in [0, num_nodes)."""
    ei = _as_pairs(edge_index)
    if ei.numel() and (int(ei.min()) < 0 or int(ei.max()) >= num_nodes):
        raise ValueError(f"edge_index holds a node outside [0, {num_nodes})")
    return ei


# ---- structure -----------------------------------------------------------------------------------------------------
def ptr_of(key, n):
    """int64 [n + 1]: ptr[i] = entries of `key` below i."""
    p = torch.zeros(n + 1, dtype=torch.int64, device=key.device)
    p[1:] = torch.cumsum(torch.bincount(key, minlength=n), 0)
    return p


def csr_both(src, dst, n, nbr_of):
    """(in_ptr, in_nbr, perm_in, out_ptr, out_nbr, perm_out) of the arcs src -> dst over n nodes: the CSR by
    destination and the one by source, every list in a fixed order (by the other end, duplicates in input order).
    perm_* is the arc of every CSR entry; nbr_of maps a node to what the kernel reads as its neighbour id."""
    perm_in = torch.sort(dst * n + src, stable=True).indices
    perm_out = torch.sort(src * n + dst, stable=True).indices
    return (ptr_of(dst, n), nbr_of(src[perm_in]).contiguous(), perm_in,
            ptr_of(src, n), nbr_of(dst[perm_out]).contiguous(), perm_out)


def split_arcs(subs):
    """(src, dst, weight, loc, n) of a `SubgraphList`: its arcs over the split's n nodes (int64 [Σe], the stored
    weights beside them) and every node's position in its own subgraph (int32 [n])."""
    s = subs.subs
    dev = s.node_ptr.device
    n, e, L = subs._node_ptr[-1], subs._edge_ptr[-1], len(subs)
    links = torch.arange(L, device=dev)
    first = s.node_ptr[:-1]
    first_e = first[torch.repeat_interleave(links, s.edge_ptr.diff(), output_size=e)]
    node = torch.arange(n, device=dev)
    loc = (node - first[torch.repeat_interleave(links, s.node_ptr.diff(), output_size=n)]).to(torch.int32)
    return s.src.long() + first_e, s.dst.long() + first_e, s.weight, loc, n


def graph_arcs(edge_index, num_nodes, device=None):
    """(src, dst, None, loc, n) of a whole graph (edge_index [2, E], flow source -> target) on the engine's device:
    one subgraph holding every node, loc = arange(n)."""
    n = int(num_nodes)
    ei = check_ids(edge_index, n)
    if n >= 2**31:
        raise ValueError("a whole-graph operator indexes nodes with int32: at most 2^31 - 1 nodes")
    dev = default_engine(device).device
    ei = ei.to(device=dev, dtype=torch.int64)
    return ei[0], ei[1], None, torch.arange(n, dtype=torch.int32, device=dev), n


def add_remaining_self_loops(src, dst, weight, n):
    """PyG add_remaining_self_loops with fill 1: the (i, i) entries leave the list and every node gets one loop at
    the end, in node order; with weights, a dropped loop's weight becomes its node's loop weight (fp32)."""
    node = torch.arange(n, device=src.device)
    loop = src == dst
    keep = ~loop
    w = None
    if weight is not None:
        wl = torch.ones(n, dtype=torch.float32, device=src.device)
        wl[src[loop]] = weight[loop].float()
        w = torch.cat([weight[keep].float(), wl])
    return torch.cat([src[keep], node]), torch.cat([dst[keep], node]), w


def gic_arcs(src, dst, n):
    """(src, dst, coef) of CalGIC's operator D·(A + I)ᵀ·D over n nodes, A[src, dst] += 1 per input arc (to_scipy_
    sparse_matrix: duplicates add up, an (i, i) entry stays): the input arcs followed by one loop per node, with
    coef = d[src]·d[dst] (fp64) and d = rowsum(A + I)^-1/2 = (out-degree + 1)^-1/2, never zero.
    out[i] = Σ_arcs j -> i coef·h[j].  Pure tensor code: runs on any device."""
    node = torch.arange(n, device=src.device)
    d = (torch.bincount(src, minlength=n).to(torch.float64) + 1.0).pow(-0.5)
    s, t = torch.cat([src, node]), torch.cat([dst, node])
    return s, t, d[s] * d[t]


# ---- the operator kinds ----------------------------------------------------------------------------------------
class _GcnOperator:
    def _build(self, src, dst, weight, loc, n, device):
        src, dst, w = add_remaining_self_loops(src, dst, weight, n)
        self.in_ptr, self.in_nbr, perm_in, self.out_ptr, self.out_nbr, perm_out = \
            csr_both(src, dst, n, lambda ids: loc[ids])
        self.dinv = torch.empty(n, dtype=torch.float32, device=loc.device)
        if n:
            eng = default_engine(device)
            N.check(N.lib().s3grl_gcn_norm(eng._ctx, n, N.ptr(self.in_ptr),
                                           N.ptr(w[perm_in] if w is not None else None), N.ptr(self.dinv)),
                    "s3grl_gcn_norm")
        coef = self.dinv[src] * w * self.dinv[dst] if w is not None else self.dinv[src] * self.dinv[dst]
        self.in_coef = coef[perm_in].contiguous()
        self.out_coef = coef[perm_out].contiguous()
        self.loc, self.num_nodes, self.use_edge_weight = loc, n, w is not None


class _RawOperator:
    def _build(self, src, dst, _weight, loc, n):
        self.in_ptr, self.in_nbr, _, self.out_ptr, self.out_nbr, _ = csr_both(src, dst, n, lambda ids: loc[ids])
        self.scale = (1.0 / self.in_ptr.diff().clamp(min=1).to(torch.float32)).contiguous()
        self.loc, self.num_nodes = loc, n


class GcnSplit(_GcnOperator):
    """The GCN operator of a whole split (every node of a `SubgraphList`), device tensors built once:
    edges into a node (forward) and out of it (backward) as CSR over the split's nodes, the neighbour as a
    position inside its own subgraph, and coef = dinv[src] · w · dinv[dst] in both orders."""

    def __init__(self, subs, use_edge_weight=False):
        src, dst, weight, loc, n = split_arcs(subs)
        self._build(src, dst, weight if use_edge_weight else None, loc, n, loc.device)


class GcnGraph(_GcnOperator):
    """GCNConv's operator over a whole graph (edge_index [2, E], flow source -> target, add_remaining_self_loops with
    fill 1), laid out as the `GcnSplit` of one subgraph holding every node: rows = loc = arange(N), nbr = the
    global id.  Built once per graph; s3grl_gcn_norm and s3grl_gcn_propagate run on it unchanged."""

    def __init__(self, edge_index, num_nodes, device=None):
        self._build(*graph_arcs(edge_index, num_nodes, device), device)
        self.rows = torch.arange(self.num_nodes, device=self.loc.device)

    def propagate(self, h, bias=None):
        """out [N, H] = Σ_{j -> i, self-loop included} dinv[j]·dinv[i]·h[j] (+ bias), differentiable in h and bias."""
        if not h.is_cuda:
            raise RuntimeError("GCN propagation runs on the MI355X only; there is no CPU fallback")
        if h.dtype != torch.float32 or h.dim() != 2 or h.shape[0] != self.num_nodes:
            raise ValueError(f"h must be float32 [{self.num_nodes}, H]")
        return _GcnPropagate.apply(h.contiguous(), bias, self.rows, self)


class GicGraph:
    """Graph InfoClust's operator over a whole graph (edge_index [2, E], flow source -> target): normalize_adj(A + I)
    of reference GICEmbs.py:CalGIC as `gic_arcs` states it, laid out like `GcnGraph` (rows = loc = arange(N)) so
    that s3grl_gcn_propagate runs on it unchanged.  Equal to `GcnGraph` on a symmetric edge_index without loops;
    different on one-directional edges, duplicates or loops.  Built once per graph."""

    def __init__(self, edge_index, num_nodes, device=None):
        src, dst, _, loc, n = graph_arcs(edge_index, num_nodes, device)
        src, dst, coef = gic_arcs(src, dst, n)
        coef = coef.to(torch.float32)
        self.in_ptr, self.in_nbr, perm_in, self.out_ptr, self.out_nbr, perm_out = \
            csr_both(src, dst, n, lambda ids: loc[ids])
        self.in_coef = coef[perm_in].contiguous()
        self.out_coef = coef[perm_out].contiguous()
        self.loc, self.num_nodes = loc, n
        self.rows = torch.arange(n, device=loc.device)

    def propagate(self, h, bias=None):
        """out [N, H] = Σ_{arc j -> i} d[j]·d[i]·h[j] + d[i]²·h[i] (+ bias), differentiable in h and bias."""
        if not h.is_cuda:
            raise RuntimeError("GIC propagation runs on the MI355X only; there is no CPU fallback")
        if h.dtype != torch.float32 or h.dim() != 2 or h.shape[0] != self.num_nodes:
            raise ValueError(f"h must be float32 [{self.num_nodes}, H]")
        return _GcnPropagate.apply(h.contiguous(), bias, self.rows, self)


class NbrSplit(_RawOperator):
    """The raw-edge operator of a whole split (every node of a `SubgraphList`), device tensors built once: the arcs
    into a node (forward) and out of it (backward) as CSR over the split's nodes, the neighbour as a position inside
    its own subgraph, and scale = 1 / max(in-degree, 1) for the mean."""

    def __init__(self, subs):
        self._build(*split_arcs(subs))


class NbrGraph(_RawOperator):
    """The raw-edge operator of a whole graph (edge_index [2, E], flow source -> target), laid out as the `NbrSplit`
    of one subgraph holding every node: rows = loc = arange(N), nbr = the global id.  Built once per graph."""

    def __init__(self, edge_index, num_nodes, device=None):
        arcs = graph_arcs(edge_index, num_nodes, device)
        self._build(*arcs)
        self.edge_index = torch.stack(arcs[:2])
        self.rows = torch.arange(self.num_nodes, device=self.loc.device)


# ---- GCN propagation -----------------------------------------------------------------------------------------------
def _propagate(eng, rows, split, forward, h, bias):
    """h (or the upstream gradient) and bias contiguous; float4 loads want them 16-byte aligned too."""
    h = N.aligned16(h)
    bias = N.aligned16(bias) if bias is not None else None
    out = torch.empty_like(h)
    ptr, nbr, coef = ((split.in_ptr, split.in_nbr, split.in_coef) if forward else
                      (split.out_ptr, split.out_nbr, split.out_coef))
    N.check(N.lib().s3grl_gcn_propagate(eng._ctx, h.shape[0], h.shape[1], N.ptr(rows), N.ptr(split.loc), N.ptr(ptr),
                                        N.ptr(nbr), N.ptr(coef), N.ptr(h), N.ptr(bias), N.ptr(out)),
            "s3grl_gcn_propagate")
    return out


class _GcnPropagate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, bias, rows, split):
        eng = default_engine(h.device)
        ctx.rows, ctx.split = rows, split
        ctx.has_bias = bias is not None
        return _propagate(eng, rows, split, True, h.contiguous(), bias.contiguous() if bias is not None else None)

    @staticmethod
    def backward(ctx, grad_out):
        eng = default_engine(grad_out.device)
        grad_out = grad_out.contiguous()
        gh = _propagate(eng, ctx.rows, ctx.split, False, grad_out, None) if ctx.needs_input_grad[0] else None
        gb = grad_out.sum(0) if ctx.has_bias and ctx.needs_input_grad[1] else None
        return gh, gb, None, None


def gcn_propagate(h, batch, bias=None):
    """out [n, H] = Σ_{j -> i, self-loop included} dinv[j] · w_ji · dinv[i] · h[j] (+ bias): GCNConv's
    propagation of h = lin(x) [n, H] fp32 over the subgraphs of `batch` (`SubgraphList.batch`)."""
    if not h.is_cuda:
        raise RuntimeError("gcn_propagate runs on the MI355X only; there is no CPU fallback")
    if h.dtype != torch.float32 or h.dim() != 2 or h.shape[0] != batch.num_nodes:
        raise ValueError("h must be float32 [batch.num_nodes, H]")
    if bias is not None and (bias.dtype != torch.float32 or bias.shape != (h.shape[1],)):
        raise ValueError("bias must be float32 [H]")
    return _GcnPropagate.apply(h, bias, batch.rows, batch.gcn)


# ---- raw-edge aggregation ------------------------------------------------------------------------------------------
def _run_aggregate(rows, split, forward, mean, self_coef, h):
    eng = default_engine(h.device)
    h = N.aligned16(h)                     # float4 loads: 16-byte aligned rows
    out = torch.empty_like(h)
    ptr, nbr = (split.in_ptr, split.in_nbr) if forward else (split.out_ptr, split.out_nbr)
    side = N.SCALE_NONE if not mean else (N.SCALE_OWN if forward else N.SCALE_NEIGHBOUR)
    N.check(N.lib().s3grl_nbr_aggregate(eng._ctx, h.shape[0], h.shape[1], N.ptr(rows), N.ptr(split.loc), N.ptr(ptr),
                                        N.ptr(nbr), N.ptr(split.scale if mean else None), side, float(self_coef),
                                        N.ptr(h), N.ptr(out)), "s3grl_nbr_aggregate")
    return out


class _NbrAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, rows, split, mean, self_coef):
        ctx.rows, ctx.split, ctx.mean, ctx.self_coef = rows, split, mean, self_coef
        return _run_aggregate(rows, split, True, mean, self_coef, h.contiguous())

    @staticmethod
    def backward(ctx, grad_out):
        gh = _run_aggregate(ctx.rows, ctx.split, False, ctx.mean, ctx.self_coef, grad_out.contiguous())
        return gh, None, None, None, None


def _operator(op):
    """(rows, split) of a `SealBatch` or an `NbrGraph`."""
    if isinstance(op, NbrGraph):
        return op.rows, op
    split = getattr(op, "nbr", None)
    if not isinstance(split, NbrSplit):
        raise TypeError("op must be a SubgraphList.batch(...) or an NbrGraph")
    return op.rows, split


def aggregate(h, op, mode, self_coef=0.0):
    """out [n, H] = self_coef · h[i] + Σ_{j -> i} h[j] (mode "sum") or self_coef · h[i] + mean_{j -> i} h[j] (mode
    "mean", a zero mean for a node without in-arcs) of h [n, H] fp32 over the raw edge list of `op`: a batch of
    `SubgraphList.batch` or an `NbrGraph`.  Differentiable in h; self_coef is a host float."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    if not h.is_cuda:
        raise RuntimeError("aggregate runs on the MI355X only; there is no CPU fallback")
    if h.dtype != torch.float32 or h.dim() != 2 or h.shape[0] != op.num_nodes:
        raise ValueError("h must be float32 [op.num_nodes, H]")
    rows, split = _operator(op)
    return _NbrAggregate.apply(h, rows, split, mode == "mean", float(self_coef))
