"""Neural Common Neighbour link prediction (NCN; Wang et al., ICLR 2024): a pair is scored from whole-graph message
passing plus the pooled embeddings of the pair's common neighbours.  The operator C[l] = Σ_{w ∈ N(u_l) ∩ N(v_l)} Z[w],
differentiable in Z, runs as HIP kernels in csrc/s3grl_ncn.hip behind the C ABI s3grl_cn_count / s3grl_cn_fill /
s3grl_segment_sum; DESIGN.md §26 is the specification (the reference has no NCN) and tests/ncn_reference.py restates
it in numpy.

    cn = CommonNeighbours(A, links)              # every link's common-neighbour list, on the device
    cn.ptr, cn.idx, cn.counts                    # int64 [L+1], int32 [Σ|CN|] ascending per link, int64 [L]
    cn.t_ptr, cn.t_link                          # the transpose (lazy): per node the links whose list holds it
    C = common_neighbour_sum(z, cn)              # fp32 [L, H], differentiable in z
    results = run_ncn(split)                     # {'AUC': (val, test), 'AP': (val, test)} of an NCNTwin

`A` is taken as `heuristics.canonical_csr` takes it and used structurally: N(x) is the stored keys of row x, values
are ignored and nothing is symmetrised.  A device triple (ptr int64 [N+1], idx int32 [nnz], N) with sorted, distinct
rows is taken as it is, so that a masked CSR made on the device needs no host trip.  `exclude_endpoints` drops u and v
from the list of (u, v): exactly what removing the link's own entries (u, v) and (v, u) does to the set, since an
endpoint can only be its own common neighbour through a self-loop.

The order of the fp32 additions is part of the specification (chunks of 64 entries, each summed from its first entry,
the partials summed in chunk order): forward and gradient are bit-identical between runs and equal to the restatement.
GPU only; there is no CPU fallback.  Node ids outside [0, N) raise ValueError before any GPU work.

NCNC, the paper's completion step (restated in tests/ncnc_reference.py), also pools the neighbours that
only one endpoint has, each weighted by the probability, predicted by NCN itself, that its missing edge exists:

    sn = SplitNeighbours(A, links)               # per link N(u) ∩ N(v), N(u) − N(v), N(v) − N(u), one after the other
    sn.ptr, sn.idx, sn.side, sn.counts           # int64 [L+1], int32, int32 (0 / 1 / 2), int64 [3, L]
    sn.inner_links, sn.inner_at                  # the pairs to complete, (w, v) or (u, w), and their entries
    C = completed_neighbour_sum(z, sn, weights)  # fp32 [L, H] = Σ weights[j]·z[idx[j]], differentiable in z and weights
    results = run_ncnc(split)                    # the same dict, of an NCNCTwin
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _native as N
from . import gae
from .heuristics import canonical_csr, check_links
from .mpgnn import NetTwin, _linear_init
from .propagate import ptr_of

CHUNK = 64      # kChunk of csrc/s3grl_ncn.hip: entries per partial sum


def check_flag(exclude_endpoints):
    """exclude_endpoints as the kernels take it (0 or 1); ValueError for anything but a bool or 0 / 1."""
    if isinstance(exclude_endpoints, (bool, np.bool_)) or (isinstance(exclude_endpoints, (int, np.integer))
                                                          and exclude_endpoints in (0, 1)):
        return int(exclude_endpoints)
    raise ValueError(f"exclude_endpoints must be a bool, got {exclude_endpoints!r}")


def check_size(num_nodes, num_entries):
    if not 1 <= num_nodes < 1 << 31 or not 0 <= num_entries < 1 << 31:
        raise ValueError(f"need 1 <= N < 2^31 and nnz < 2^31, got N = {num_nodes}, nnz = {num_entries}")


def _graph_on(A_or_csr, engine_for):
    """(ptr int64 [N+1], idx int32 [nnz], N, engine) on the device, from a scipy matrix or a device triple."""
    if isinstance(A_or_csr, (tuple, list)):
        if len(A_or_csr) != 3:
            raise ValueError("a device CSR is the triple (ptr, idx, N)")
        ptr, idx, n = A_or_csr
        n = int(n)
        if not (isinstance(ptr, torch.Tensor) and isinstance(idx, torch.Tensor)):
            raise ValueError("a device CSR is the triple (ptr, idx, N) of two tensors and an int")
        if ptr.dtype != torch.int64 or idx.dtype != torch.int32 or ptr.dim() != 1 or idx.dim() != 1 or \
                ptr.numel() != n + 1:
            raise ValueError("a device CSR needs ptr int64 [N + 1] and idx int32 [nnz]")
        check_size(n, idx.numel())
        if not ptr.is_cuda or ptr.device != idx.device:
            raise RuntimeError("common-neighbour lists need a HIP device (MI355X); there is no CPU fallback")
        eng = engine_for(ptr.device)
        rising = bool((ptr[1:] >= ptr[:-1]).all()) and int(ptr[0]) == 0 and int(ptr[-1]) == idx.numel()
        if not rising or (idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n)):
            raise ValueError("malformed CSR (ptr not monotone from 0 to nnz, or a column outside [0, N))")
        return ptr.contiguous(), idx.contiguous(), n, eng
    A = canonical_csr(A_or_csr)
    check_size(A.shape[0], A.nnz)
    eng = engine_for(None)
    dev = eng.device
    return (torch.as_tensor(A.indptr.astype(np.int64)).to(dev), torch.as_tensor(A.indices.astype(np.int32)).to(dev),
            A.shape[0], eng)


def _links_on(links, num_nodes, dev):
    """links [2, L] as int32 on the device; ValueError on a bad shape or a node outside [0, N).  A device tensor is
    checked on the device."""
    if isinstance(links, torch.Tensor) and links.is_cuda:
        if links.numel() == 0:
            return torch.zeros((2, 0), dtype=torch.int32, device=dev)
        if links.dim() != 2 or links.shape[0] != 2:
            raise ValueError(f"edge_index must be [2, L], got {tuple(links.shape)}")
        if links.dtype.is_floating_point or links.dtype == torch.bool:
            raise ValueError(f"edge_index must hold integer node ids, got {links.dtype}")
        if int(links.min()) < 0 or int(links.max()) >= num_nodes:
            raise ValueError(f"edge_index holds a node outside [0, {num_nodes})")
        return links.to(device=dev, dtype=torch.int32).contiguous()
    return torch.as_tensor(check_links(links, num_nodes).astype(np.int32)).to(dev).contiguous()


class SegmentLists:
    """R lists of rows of an [M, H] matrix: ptr int64 [R+1], idx int32 [ptr[R]], on the device, and lazily the
    transpose: t_ptr int64 [M+1] and t_link int32, per row of the matrix the lists that hold it, in ascending list
    index (a stable sort of idx with each entry's list carried along, as `propagate.csr_both` sorts), and t_perm int64,
    the entry that each transposed position came from: a vector with a value per entry is taken to transposed order by
    `values[t_perm]`."""

    def __init__(self, ptr, idx, num_source_rows):
        self.ptr, self.idx, self.num_source_rows = ptr, idx, int(num_source_rows)
        self._t = None

    def __len__(self):
        return self.ptr.numel() - 1

    def _transpose(self):
        if self._t is None:
            L, dev = len(self), self.ptr.device
            owner = torch.repeat_interleave(torch.arange(L, device=dev), self.ptr.diff(), output_size=self.idx.numel())
            keys = self.idx.long()
            order = torch.sort(keys, stable=True).indices
            self._t = (ptr_of(keys, self.num_source_rows), owner[order].to(torch.int32).contiguous(), order)
        return self._t

    @property
    def t_ptr(self):
        return self._transpose()[0]

    @property
    def t_link(self):
        return self._transpose()[1]

    @property
    def t_perm(self):
        return self._transpose()[2]


class CommonNeighbours(SegmentLists):
    """The common-neighbour list of every link of `links` [2, L] on the graph `A_or_csr` (a scipy matrix or a device
    (ptr, idx, N) triple): N(u) ∩ N(v) in ascending id, less u and v themselves with `exclude_endpoints`.  u == v
    gives N(u); repeated links give repeated lists.  `.ptr`, `.idx`, `.counts` and the lazy `.t_ptr`, `.t_link` are
    device tensors; `.counts` equals `Heuristics.cn` on a 0/1 graph without self-loops at the endpoints."""

    def __init__(self, A_or_csr, links, exclude_endpoints=True, device=None):
        flag = check_flag(exclude_endpoints)
        if device is not None and torch.device(device).type == "cpu":
            raise RuntimeError("common-neighbour lists need a HIP device (MI355X); there is no CPU fallback")
        from .engine import default_engine

        gp, gi, n, eng = _graph_on(A_or_csr, lambda d: default_engine(d if d is not None else device))
        dev = eng.device
        ei = _links_on(links, n, dev)
        L = ei.shape[1]
        self.engine, self.num_nodes, self.links, self.exclude_endpoints = eng, n, ei, bool(flag)
        self.counts = torch.empty(L, dtype=torch.int64, device=dev)
        N.check(N.lib().s3grl_cn_count(eng._ctx, n, N.ptr(gp), N.ptr(gi), gi.numel(), N.ptr(ei), L, flag,
                                       N.ptr(self.counts)), "s3grl_cn_count")
        ptr = torch.zeros(L + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(self.counts, 0)
        total = int(ptr[-1])
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        N.check(N.lib().s3grl_cn_fill(eng._ctx, n, N.ptr(gp), N.ptr(gi), gi.numel(), N.ptr(ei), L, flag, N.ptr(ptr),
                                      total, N.ptr(idx)), "s3grl_cn_fill")
        super().__init__(ptr, idx, n)


def _segment_sum(h, ptr, idx, num_rows):
    """out [R, H] of the kernel; h fp32 [M, H] contiguous on the device, the lists trusted."""
    from .engine import default_engine

    eng = default_engine(h.device)
    out = torch.empty((num_rows, h.shape[1]), dtype=torch.float32, device=h.device)
    N.check(N.lib().s3grl_segment_sum(eng._ctx, N.ptr(h), h.shape[0], h.shape[1], N.ptr(ptr), N.ptr(idx), num_rows,
                                      N.ptr(out)), "s3grl_segment_sum")
    return out


def segment_sum(h, ptr, idx):
    """out[r, :] = Σ_j h[idx[j], :] over j in [ptr[r], ptr[r+1]) in the order DESIGN.md §26 fixes: h fp32 [M, H], ptr
    int64 [R+1], idx int32, all on the device -> fp32 [R, H].  Not differentiable (`common_neighbour_sum` is); the
    lists are checked on the device first (ValueError)."""
    if not h.is_cuda:
        raise RuntimeError("segment_sum runs on the MI355X only; there is no CPU fallback")
    if h.dtype != torch.float32 or h.dim() != 2 or h.shape[1] < 1:
        raise ValueError("h must be float32 [M, H] with H >= 1")
    if ptr.dtype != torch.int64 or idx.dtype != torch.int32 or ptr.dim() != 1 or idx.dim() != 1 or ptr.numel() < 1:
        raise ValueError("need ptr int64 [R + 1] and idx int32")
    if int(ptr[0]) != 0 or int(ptr[-1]) != idx.numel() or not bool((ptr[1:] >= ptr[:-1]).all()) or \
            (idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= h.shape[0])):
        raise ValueError("malformed lists (ptr not monotone from 0 to len(idx), or an entry outside [0, M))")
    return _segment_sum(h.contiguous(), ptr.contiguous(), idx.contiguous(), ptr.numel() - 1)


class _ListSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, lists):
        ctx.lists = lists
        return _segment_sum(z.contiguous(), lists.ptr, lists.idx, len(lists))

    @staticmethod
    def backward(ctx, grad_out):
        lists = ctx.lists
        return _segment_sum(grad_out.contiguous(), lists.t_ptr, lists.t_link, lists.num_source_rows), None


def common_neighbour_sum(z, cn):
    """C [L, H] = Σ_{w ∈ cn's list of l} z[w] of z [N, H] fp32 over a `CommonNeighbours` (any `SegmentLists`), summed
    in the order DESIGN.md §26 fixes; an empty list gives +0.0.  Differentiable in z: the gradient of z[w] is the sum
    of the upstream rows of the links whose list holds w, in ascending link index, in the same chunked order."""
    if not isinstance(cn, SegmentLists):
        raise TypeError("cn must be a CommonNeighbours")
    if not z.is_cuda:
        raise RuntimeError("common_neighbour_sum runs on the MI355X only; there is no CPU fallback")
    if z.dtype != torch.float32 or z.dim() != 2 or z.shape[0] != cn.num_source_rows:
        raise ValueError("z must be float32 [cn.num_nodes, H]")
    return _ListSum.apply(z, cn)


def endpoint_rows(z, ids):
    """z[ids] ([L, H]) through the same operator, as lists of one entry: the gradient is summed in ascending link
    index, bit-identical between runs."""
    L = ids.numel()
    lists = SegmentLists(torch.arange(L + 1, dtype=torch.int64, device=ids.device),
                         ids.to(torch.int32).contiguous(), z.shape[0])
    return _ListSum.apply(z, lists)


# ---- NCNC: split lists, the weighted sum and its two gradients -----------------------------------------------------
class SplitNeighbours(SegmentLists):
    """Per link (u, v) of `links` [2, L] the three sections S0 = N(u) ∩ N(v), S1 = N(u) \\ N(v), S2 = N(v) \\ N(u),
    each in ascending id, one after the other; `exclude_endpoints` drops the keys u and v from all three.  u == v gives
    S0 = N(u) and empty S1, S2.  `.ptr` int64 [L+1], `.idx` int32 and `.side` int32 (the section of every entry),
    `.counts` int64 [3, L]; `.inner_at` int64, the positions of the S1 and S2 entries, and `.inner_links` int32
    [2, n_inner], the pair each of them stands for: (w, v) for w in S1 (u has the edge, v's is the one to complete) and
    (u, w) for w in S2, in entry order.  `.csr` is the graph's device triple.  All on the device."""

    def __init__(self, A_or_csr, links, exclude_endpoints=True, device=None):
        flag = check_flag(exclude_endpoints)
        if device is not None and torch.device(device).type == "cpu":
            raise RuntimeError("split neighbour lists need a HIP device (MI355X); there is no CPU fallback")
        from .engine import default_engine

        gp, gi, n, eng = _graph_on(A_or_csr, lambda d: default_engine(d if d is not None else device))
        dev = eng.device
        ei = _links_on(links, n, dev)
        L = ei.shape[1]
        self.engine, self.num_nodes, self.links, self.exclude_endpoints = eng, n, ei, bool(flag)
        self.csr = (gp, gi, n)
        self.counts = torch.empty((3, L), dtype=torch.int64, device=dev)
        N.check(N.lib().s3grl_cn_split_count(eng._ctx, n, N.ptr(gp), N.ptr(gi), gi.numel(), N.ptr(ei), L, flag,
                                             N.ptr(self.counts)), "s3grl_cn_split_count")
        ptr = torch.zeros(L + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(self.counts.sum(0), 0)
        total = int(ptr[-1])
        idx = torch.empty(total, dtype=torch.int32, device=dev)
        self.side = torch.empty(total, dtype=torch.int32, device=dev)
        N.check(N.lib().s3grl_cn_split_fill(eng._ctx, n, N.ptr(gp), N.ptr(gi), gi.numel(), N.ptr(ei), L, flag,
                                            N.ptr(self.counts), N.ptr(ptr), total, N.ptr(idx), N.ptr(self.side)),
                "s3grl_cn_split_fill")
        super().__init__(ptr, idx, n)
        self._inner = None

    def _inner_pairs(self):
        if self._inner is None:
            at = torch.nonzero(self.side).reshape(-1)
            owner = torch.searchsorted(self.ptr, at, right=True) - 1
            w, first = self.idx[at], self.side[at] == 1
            u, v = self.links[0][owner], self.links[1][owner]
            self._inner = (at, torch.stack([torch.where(first, w, u), torch.where(first, v, w)]).contiguous())
        return self._inner

    @property
    def inner_at(self):
        return self._inner_pairs()[0]

    @property
    def inner_links(self):
        return self._inner_pairs()[1]


def _segment_wsum(h, ptr, idx, w, num_rows):
    """out [R, H] of the weighted kernel; h fp32 [M, H] and w fp32 [len(idx)] contiguous on the device."""
    from .engine import default_engine

    eng = default_engine(h.device)
    out = torch.empty((num_rows, h.shape[1]), dtype=torch.float32, device=h.device)
    N.check(N.lib().s3grl_segment_wsum(eng._ctx, N.ptr(h), h.shape[0], h.shape[1], N.ptr(ptr), N.ptr(idx), N.ptr(w),
                                       num_rows, N.ptr(out)), "s3grl_segment_wsum")
    return out


def _segment_dot(g, h, ptr, idx):
    """out_w [len(idx)]: every entry's <g[its list], h[idx]>; g fp32 [R, H], h fp32 [M, H] contiguous on the device."""
    from .engine import default_engine

    eng = default_engine(h.device)
    out = torch.empty(idx.numel(), dtype=torch.float32, device=h.device)
    N.check(N.lib().s3grl_segment_dot(eng._ctx, N.ptr(g), g.shape[0], N.ptr(h), h.shape[0], h.shape[1], N.ptr(ptr),
                                      N.ptr(idx), N.ptr(out)), "s3grl_segment_dot")
    return out


class _WeightedListSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, weights, lists):
        z, weights = z.contiguous(), weights.contiguous()
        ctx.lists = lists
        ctx.save_for_backward(z, weights)
        return _segment_wsum(z, lists.ptr, lists.idx, weights, len(lists))

    @staticmethod
    def backward(ctx, grad_out):
        lists = ctx.lists
        z, weights = ctx.saved_tensors
        g = grad_out.contiguous()
        grad_z = grad_w = None
        if ctx.needs_input_grad[0]:
            grad_z = _segment_wsum(g, lists.t_ptr, lists.t_link, weights[lists.t_perm].contiguous(),
                                   lists.num_source_rows)
        if ctx.needs_input_grad[1]:
            grad_w = _segment_dot(g, z, lists.ptr, lists.idx)
        return grad_z, grad_w, None


def completed_neighbour_sum(z, lists, weights):
    """C [L, H] = Σ_j weights[j]·z[idx[j]] over the entries j of every list of a `SplitNeighbours` (any
    `SegmentLists`): z fp32 [N, H], weights fp32 with one value per entry.  Every product is rounded once and the terms
    are added in the order DESIGN.md §26 fixes, so unit weights give `common_neighbour_sum`'s bits.  Differentiable in z
    (the same sum over the transposed lists with the weights in transposed order) and in weights (one dot product per
    entry, in the fixed order of DESIGN.md §27); both are bit-identical between runs."""
    if not isinstance(lists, SegmentLists):
        raise TypeError("lists must be a SplitNeighbours")
    if not isinstance(z, torch.Tensor) or not isinstance(weights, torch.Tensor):
        raise TypeError("z and weights must be tensors")
    if not z.is_cuda or not weights.is_cuda:
        raise RuntimeError("completed_neighbour_sum runs on the MI355X only; there is no CPU fallback")
    if z.dtype != torch.float32 or z.dim() != 2 or z.shape[0] != lists.num_source_rows:
        raise ValueError("z must be float32 [lists.num_nodes, H]")
    if weights.dtype != torch.float32 or weights.dim() != 1 or weights.numel() != lists.idx.numel():
        raise ValueError("weights must be float32 with one value per list entry")
    return _WeightedListSum.apply(z, weights, lists)


# ---- model ---------------------------------------------------------------------------------------------------------
class _MLP2(nn.Module):
    """Linear -> ReLU -> dropout -> Linear, torch's Linear init drawn from `gen`."""

    def __init__(self, a, b, c, dropout, gen):
        super().__init__()
        self.lin1, self.lin2, self.dropout = nn.Linear(a, b), nn.Linear(b, c), float(dropout)
        _linear_init(self.lin1, gen)
        _linear_init(self.lin2, gen)

    def forward(self, x):
        return self.lin2(F.dropout(self.lin1(x).relu(), self.dropout, self.training))


class NCNTwin(nn.Module):
    """NCN's predictor on a three-layer GCN encoder (`mpgnn.NetTwin(..., "GCN")`; x = None: identity features):
    xij = MLP₂(z_u ⊙ z_v), xcn = MLP₂(C) with C the summed embeddings of the common neighbours, and
    logit = MLP₂→1(xij + β·xcn), β a learnable scalar initialised to 1."""

    def __init__(self, in_channels, hidden=256, dropout=0.5, seed=0):
        super().__init__()
        if int(in_channels) < 1 or int(hidden) < 1 or not 0.0 <= float(dropout) < 1.0:
            raise ValueError("need in_channels >= 1, hidden >= 1 and 0 <= dropout < 1")
        self.hidden, self.dropout = int(hidden), float(dropout)
        self.encoder = NetTwin(int(in_channels), self.hidden, "GCN", seed=seed)
        gen = torch.Generator().manual_seed(int(seed) + 1)
        self.xij = _MLP2(self.hidden, self.hidden, self.hidden, self.dropout, gen)
        self.xcn = _MLP2(self.hidden, self.hidden, self.hidden, self.dropout, gen)
        self.out = _MLP2(self.hidden, self.hidden, 1, self.dropout, gen)
        self.beta = nn.Parameter(torch.ones(()))

    def encode(self, x, graph):
        return self.encoder.encode(x, graph, self.dropout)

    def forward(self, z, cn, use_cn=True):
        """z fp32 [N, hidden], cn a `CommonNeighbours` of the links to score -> logits fp32 [L].  `use_cn=False`
        zeroes the CN branch: a plain GCN + MLP decoder."""
        u, v = cn.links[0], cn.links[1]
        h = self.xij(endpoint_rows(z, u) * endpoint_rows(z, v))
        if use_cn:
            h = h + self.beta * self.xcn(common_neighbour_sum(z, cn))
        return self.out(h).reshape(-1)


class NCNCTwin(NCNTwin):
    """NCNC: NCN with its common-neighbour pool completed.  The parameters and their names are NCNTwin's (`encoder`,
    `xij`, `xcn`, `out`, `beta`), so a trained NCN `state_dict` loads.  For a link (u, v), a neighbour w of u alone
    enters the pool with weight p(w, v) and a neighbour of v alone with p(u, w), where p is the sigmoid of the NCN
    forward of that inner pair on the same z and graph with the same weights; common neighbours enter with weight 1.
    With `detach_completion` no gradient flows through p."""

    def __init__(self, in_channels, hidden=256, dropout=0.5, seed=0, detach_completion=False):
        super().__init__(in_channels, hidden, dropout, seed)
        self.detach_completion = bool(detach_completion)

    def completion_weights(self, z, sn):
        """fp32 [len(sn.idx)]: 1 on S0, p of the inner pair on S1 and S2"""
        ones = torch.ones(sn.idx.numel(), dtype=torch.float32, device=z.device)
        at = sn.inner_at
        if at.numel() == 0:
            return ones
        inner = CommonNeighbours(sn.csr, sn.inner_links, sn.exclude_endpoints)
        p = torch.sigmoid(NCNTwin.forward(self, z, inner))
        return ones.index_copy(0, at, p.detach() if self.detach_completion else p)

    def forward(self, z, sn):
        """z fp32 [N, hidden], sn a `SplitNeighbours` of the links to score -> logits fp32 [L]"""
        u, v = sn.links[0], sn.links[1]
        h = self.xij(endpoint_rows(z, u) * endpoint_rows(z, v))
        h = h + self.beta * self.xcn(completed_neighbour_sum(z, sn, self.completion_weights(z, sn)))
        return self.out(h).reshape(-1)


# ---- training ------------------------------------------------------------------------------------------------------
class _TrainGraph:
    """The sorted CSR of the training graph on the device, with every entry's row and key row·N + col (ascending),
    and the same graph without a batch of links, made on the device with a keep mask and a cumsum: deleting entries
    keeps rows sorted, so nothing is sorted again."""

    def __init__(self, A, device=None):
        from .engine import default_engine

        self.ptr, self.idx, self.num_nodes, self.engine = _graph_on(A, lambda d: default_engine(device))
        dev = self.engine.device
        self.row = torch.repeat_interleave(torch.arange(self.num_nodes, device=dev), self.ptr.diff(),
                                           output_size=self.idx.numel())
        self.key = self.row * self.num_nodes + self.idx.long()

    def csr(self):
        return self.ptr, self.idx, self.num_nodes

    def edge_index(self, keep=None):
        row, col = (self.row, self.idx.long()) if keep is None else (self.row[keep], self.idx[keep].long())
        return torch.stack([row, col])

    def without(self, u, v):
        """(csr triple, edge_index) of the graph less the stored entries (u_i, v_i) and (v_i, u_i)."""
        n, nnz = self.num_nodes, self.key.numel()
        if nnz == 0:
            return self.csr(), self.edge_index()
        drop = torch.cat([u.long() * n + v.long(), v.long() * n + u.long()])
        at = torch.searchsorted(self.key, drop).clamp(max=nnz - 1)
        keep = torch.ones(nnz, dtype=torch.bool, device=self.key.device)
        keep[at[self.key[at] == drop]] = False
        below = torch.zeros(nnz + 1, dtype=torch.int64, device=self.key.device)
        below[1:] = torch.cumsum(keep, 0)
        return (below[self.ptr], self.idx[keep].contiguous(), n), self.edge_index(keep)


def _train_links(model, split, x, *, epochs, lr, batch_size, seed, mask, device, history, lists_of, score,
                 eval_chunk=None):
    """The loop that `train_ncn` and `train_ncnc` share.  `lists_of(csr, links)` builds what `score(model, z, lists)`
    reads.  With `eval_chunk` None the lists of valid and test are built once, before training; with a number they are
    built anew at every evaluation for that many links at a time, so that lists far longer than the links (NCNC's inner
    pairs at hubs) never exist all at once."""
    from .metrics import LinkMetrics

    n = split.num_nodes
    g = _TrainGraph(split.A, device)
    eng = g.engine
    dev = eng.device
    model = model.to(dev)
    xs = torch.as_tensor(np.asarray(x, dtype=np.float32)).to(dev).contiguous() if x is not None else None
    if xs is not None and (xs.dim() != 2 or xs.shape[0] != n):
        raise ValueError(f"x must be [{n}, F], got {tuple(xs.shape)}")
    train_pos = torch.as_tensor(check_links(split.links["train"][0], n)).to(dev)
    avoid = gae.PairList(split.edge_index(), n, dev)            # what the negatives avoid
    avoid.keys()
    full_graph = gae.GcnGraph(g.edge_index(), n, dev)
    evals = {}
    for name in ("valid", "test"):
        pos, neg = (check_links(t, n) for t in split.links[name])
        both = np.concatenate([pos, neg], axis=1)
        if eval_chunk is None:
            evals[name] = ([lists_of(g.csr(), both)], pos.shape[1])
        else:
            both = torch.as_tensor(both).to(dev)
            evals[name] = ([both[:, c:c + eval_chunk] for c in range(0, both.shape[1], eval_chunk)], pos.shape[1])

    def evaluate(z, parts):
        logits = [score(model, z, part if eval_chunk is None else lists_of(g.csr(), part)) for part in parts]
        return logits[0] if len(logits) == 1 else torch.cat(logits)

    opt = torch.optim.Adam(model.parameters(), lr=lr)
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    torch.manual_seed(int(seed))                                # the dropout masks
    results, losses, step = {"AUC": [], "AP": []}, [], 0
    P = train_pos.shape[1]
    metrics = LinkMetrics(dev)
    try:
        for _ in range(epochs):
            model.train()
            perm = torch.randperm(P, generator=gen).to(dev)
            total = 0.0
            for b0 in range(0, P, batch_size):
                step += 1
                pos = train_pos[:, perm[b0:b0 + batch_size]]
                B = pos.shape[1]
                neg = gae._sample(avoid, B, seed, step)
                links = torch.cat([pos, torch.stack([neg.src.long(), neg.dst.long()])], dim=1)
                label = torch.cat([torch.ones(B, device=dev), torch.zeros(len(neg), device=dev)])
                if mask:
                    csr, ei = g.without(pos[0], pos[1])
                    graph = gae.GcnGraph(ei, n, dev)
                else:
                    csr, graph = g.csr(), full_graph
                opt.zero_grad(set_to_none=True)
                z = model.encode(xs, graph)
                loss = F.binary_cross_entropy_with_logits(score(model, z, lists_of(csr, links)), label)
                loss.backward()
                opt.step()
                value = loss.item()
                if history is not None:
                    history.append(value)
                total += value * B
            losses.append(total / max(P, 1))
            model.eval()
            with torch.no_grad():
                z = model.encode(xs, full_graph)
                res = {name: metrics.ranked(evaluate(z, parts), n_pos=n_pos) for name, (parts, n_pos) in evals.items()}
            for key in results:
                results[key].append((res["valid"][key], res["test"][key]))
    finally:
        metrics.close()
    return results, losses


def train_ncn(model, split, x=None, *, epochs=50, lr=0.01, batch_size=1024, seed=1, mask=True, use_cn=True,
              device=None, history=None):
    """Adam on BCE-with-logits.  Per step: a batch of shuffled train positives and as many negatives from
    `gae._sample` keyed by (seed, step); with `mask`, the batch's positives leave, in both directions, the graph that
    the encoder and the CN lists see (a masked CSR and a `GcnGraph` of the kept arcs per step).  After every epoch
    valid and test are scored on the unmasked train graph.  Returns (per-epoch {'AUC': [(val, test)], 'AP': [...]},
    the mean loss of every epoch); `history`, a list, receives every step's loss."""
    return _train_links(model, split, x, epochs=epochs, lr=lr, batch_size=batch_size, seed=seed, mask=mask,
                        device=device, history=history, lists_of=lambda csr, links: CommonNeighbours(csr, links, True),
                        score=lambda m, z, cn: m(z, cn, use_cn))


EVAL_CHUNK = 4096   # links whose split lists and inner pairs exist at once while `train_ncnc` evaluates


def train_ncnc(model, split, x=None, *, epochs=50, lr=0.01, batch_size=1024, seed=1, mask=True, device=None,
               history=None):
    """`train_ncn`'s loop on an `NCNCTwin`: the lists are `SplitNeighbours`, and valid and test are scored EVAL_CHUNK
    links at a time, their lists built anew at every evaluation."""
    return _train_links(model, split, x, epochs=epochs, lr=lr, batch_size=batch_size, seed=seed, mask=mask,
                        device=device, history=history, lists_of=lambda csr, links: SplitNeighbours(csr, links, True),
                        score=lambda m, z, sn: m(z, sn), eval_chunk=EVAL_CHUNK)


def run_ncn(split, x=None, *, epochs=50, hidden=256, lr=0.01, dropout=0.5, batch_size=1024, seed=1, mask=True,
            use_cn=True, device=None, history=None):
    """The NCN row from a `workloads.Split` (x = None is eye(N)): an `NCNTwin` trained by `train_ncn`.  `mask=True`
    removes each batch's positives from the graph the model sees, so that a train positive is scored as a test link is:
    without its own edge.  `use_cn=False` is the ablation, a plain GCN + MLP decoder.  Returns {'AUC': (best val,
    test at it), 'AP': (...)}, each at the first epoch of its own maximal val value, as fractions (like run_mpgnn)."""
    if int(epochs) < 1 or not float(lr) > 0.0 or int(batch_size) < 1 or int(hidden) < 1 or \
            not 0.0 <= float(dropout) < 1.0:
        raise ValueError("need epochs >= 1, lr > 0, batch_size >= 1, hidden >= 1 and 0 <= dropout < 1")
    dev = gae.check_device(device)
    in_channels = split.num_nodes if x is None else np.asarray(x).shape[1]
    model = NCNTwin(in_channels, int(hidden), float(dropout), seed=int(seed))
    results, _ = train_ncn(model, split, x, epochs=int(epochs), lr=float(lr), batch_size=int(batch_size),
                           seed=int(seed), mask=bool(mask), use_cn=bool(use_cn), device=dev, history=history)
    return {k: tuple(float(v) for v in gae.best_at_first_max(r)) for k, r in results.items()}


def run_ncnc(split, x=None, *, epochs=50, hidden=256, lr=0.01, dropout=0.5, batch_size=1024, seed=1, mask=True,
             device=None, history=None):
    """The NCNC row from a `workloads.Split`: an `NCNCTwin` trained by `train_ncnc`, with `run_ncn`'s arguments,
    refusals and result ({'AUC': (best val, test at it), 'AP': (...)})."""
    if int(epochs) < 1 or not float(lr) > 0.0 or int(batch_size) < 1 or int(hidden) < 1 or \
            not 0.0 <= float(dropout) < 1.0:
        raise ValueError("need epochs >= 1, lr > 0, batch_size >= 1, hidden >= 1 and 0 <= dropout < 1")
    dev = gae.check_device(device)
    in_channels = split.num_nodes if x is None else np.asarray(x).shape[1]
    model = NCNCTwin(in_channels, int(hidden), float(dropout), seed=int(seed))
    results, _ = train_ncnc(model, split, x, epochs=int(epochs), lr=float(lr), batch_size=int(batch_size),
                            seed=int(seed), mask=bool(mask), device=dev, history=history)
    return {k: tuple(float(v) for v in gae.best_at_first_max(r)) for k, r in results.items()}
