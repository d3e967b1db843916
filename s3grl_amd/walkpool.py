"""The WalkPool row of Table 2 (reference Software/WalkPooling/src/model.py, utils.py, main.py): the model's own
operator as HIP kernels behind the C ABI (s3grl_wp_*, csrc/s3grl_walkpool.hip), a twin of the model on this package's
enclosing subgraphs, and the run function of one row.

    subs = enclosing_subgraphs(link_index, A, x, 0, num_hops=2, node_label="zo")
    wps = WalkPoolSplit(subs)                                 # once per list: E+ in both arc orders, its GCN operator
    model = LinkPredTwin(32, 32, heads=2, walk_len=7, MSE=False).cuda()
    logits = model(wps.batch(link_ids))                       # [B, 1]

Per link the subgraph's local nodes 0 and 1 are the candidate link (i, j); E- is what the subgraphs hold (the induced
arcs without the candidate link), E+ = E- with i -> j and j -> i added.
  * `attention_weights(q, k, batch)`: per arc r -> c of E+ and head h the logit w = <q[r,h], k[c,h]> / sqrt(hidden);
    weights_p its softmax over the arcs of E+ into c; weights_m = mask · exp(w - max over E+ into c) / (sum over E-
    into c + 1e-16), zero on the candidate arcs; omega = sigmoid(w[i->j]) + sigmoid(w[j->i])  (model.py:74-112).
  * `walk_pool(weights_p, weights_m, batch, walk_len)`: with P[c, r] the weight of r -> c and X = P^tau, tau = 2 ..
    walk_len + 1: tr(X+) - tr(X-), X[i,i] + X[j,j] and X[i,j] + X[j,i] of both signs  (model.py:114-219).  The
    reference propagates an identity of n_total x n_max through PyG message passing; here a workgroup owns a block
    of columns in LDS and nothing of size n x n exists in HBM.
Both are deterministic (two runs are bit-identical in values and gradients).  GPU only; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _native as N
from .engine import default_engine
from .propagate import _GcnOperator, csr_both, split_arcs
from .seal import SealBatch, _to_device
from .seal_nn import GCNConv

WALK_FEATURES = 5   # graphlevel, nodelevel_p, nodelevel_m, linklevel_p, linklevel_m


def _check_walk_len(walk_len):
    if isinstance(walk_len, bool) or int(walk_len) != walk_len or not 1 <= int(walk_len) <= N.WP_MAX_WALK:
        raise ValueError(f"walk_len must be an integer in [1, {N.WP_MAX_WALK}], got {walk_len!r}")
    return int(walk_len)


def layout(n_max, e_max, heads, walk_len, lds_budget=0):
    """How the walk kernels run a batch whose largest link has n_max nodes and e_max arcs of E+ (a host function, no
    GPU): {'forward': {...}, 'backward': {...}}, each with 'block' (columns per block), 'groups' (workgroups per
    (link, head, sign)), 'flavour' ('lds' or 'hbm') and 'workspace_bytes' per link.  NotImplementedError above 4096
    nodes."""
    walk_len = _check_walk_len(walk_len)
    if int(n_max) < 0 or int(e_max) < 0 or not 1 <= int(heads) <= N.WP_MAX_HEADS or int(lds_budget) < 0:
        raise ValueError("need n_max >= 0, e_max >= 0, heads in [1, 64] and lds_budget >= 0")
    out = (C.c_int64 * 8)()
    N.check(N.lib().s3grl_wp_layout(int(n_max), int(e_max), int(heads), walk_len, int(lds_budget), out),
            "s3grl_wp_layout")
    return {name: {"block": int(out[o]), "groups": int(out[o + 1]), "flavour": "hbm" if out[o + 2] else "lds",
                   "workspace_bytes": int(out[o + 3])} for name, o in (("forward", 0), ("backward", 4))}


# ---- structure ---------------------------------------------------------------------------------------------------
class WalkPoolSplit:
    """E+ of a whole `SubgraphList`, built once: the list's arcs with the two candidate arcs of every link appended,
    grouped by target node (in_*) and by source node (out_*) over the split's nodes, the candidate flags, and the GCN
    operator of E+ (`gcn`: gcn_norm with self-loops, as `seal_nn.GCNConv` takes it).  The `SubgraphList` is not
    changed.  A link's arcs are one contiguous range of either order, `arc_ptr` (host) its bounds."""

    def __init__(self, subs):
        s = subs.subs
        src, dst, _, loc, n = split_arcs(subs)
        dev = loc.device
        L = len(subs)
        if L and int(subs.node_counts().min()) < 2:
            raise ValueError("every subgraph needs its two link nodes")
        first = s.node_ptr[:-1]
        if bool(((loc[src] < 2) & (loc[dst] < 2)).any()):
            raise ValueError("the subgraphs hold an arc between the link's own nodes: E- must not contain the link")
        src = torch.cat([src, first, first + 1])
        dst = torch.cat([dst, first + 1, first])
        flag = torch.zeros(src.numel(), dtype=torch.uint8, device=dev)
        flag[src.numel() - 2 * L:] = 1
        self.in_ptr, self.in_nbr, perm_in, self.out_ptr, self.out_nbr, perm_out = \
            csr_both(src, dst, n, lambda ids: loc[ids])
        self.in_dst = loc[dst[perm_in]].contiguous()
        self.in_flag = flag[perm_in].contiguous()
        inv = torch.empty_like(perm_in)
        inv[perm_in] = torch.arange(perm_in.numel(), device=dev)
        self.out_arc = inv[perm_out].contiguous()
        self.gcn = _GcnOperator()
        self.gcn._build(src, dst, None, loc, n, dev)
        self.subs, self.num_nodes, self.num_arcs = subs, n, int(src.numel())
        self.arc_ptr = np.asarray(subs._edge_ptr, dtype=np.int64) + 2 * np.arange(L + 1, dtype=np.int64)

    def __len__(self):
        return len(self.subs)

    def batch(self, link_ids):
        """The device batch of the links `link_ids` (host integers, in that order): what `attention_weights`,
        `walk_pool` and `seal_nn.GCNConv` take.  Sizes come from the host copies of the pointers, so nothing waits
        for the device."""
        subs = self.subs
        ids = np.asarray(link_ids, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= len(subs)):
            raise IndexError("link id outside the list")
        B = ids.size
        counts = subs._counts[ids]
        acnt = self.arc_ptr[ids + 1] - self.arc_ptr[ids]
        local, alocal = np.zeros(B + 1, dtype=np.int64), np.zeros(B + 1, dtype=np.int64)
        np.cumsum(counts, out=local[1:])
        np.cumsum(acnt, out=alocal[1:])
        n, e = int(local[-1]), int(alocal[-1])
        dev = subs.subs.node_ptr.device
        host = np.concatenate([ids, local, counts, acnt, self.arc_ptr[ids] - alocal[:-1]])
        d = _to_device(host, dev)                                             # one host -> device copy
        ids_d, ptr_d, cnt_d = d[:B], d[B:2 * B + 1], d[2 * B + 1:3 * B + 1]
        acnt_d, ashift = d[3 * B + 1:4 * B + 1], d[4 * B + 1:]
        link = torch.repeat_interleave(torch.arange(B, device=dev), cnt_d, output_size=n)
        rows = (subs.subs.node_ptr[ids_d] - ptr_d[:-1])[link] + torch.arange(n, device=dev)
        arc_shift = torch.repeat_interleave(ashift, acnt_d, output_size=e)
        arcs = arc_shift + torch.arange(e, device=dev)                        # the split's arc of every batch arc
        return WalkPoolBatch(self, ids, ids_d, rows, ptr_d, int(counts.max()) if B else 0, link, arcs, arc_shift,
                             ashift, int(acnt.max()) if B else 0)


class WalkPoolBatch(SealBatch):
    """A mini-batch of `WalkPoolSplit.batch`: a `SealBatch` whose GCN operator is that of E+ (x, z, node_ptr, rows,
    gcn, num_graphs, num_nodes, max_nodes), plus the arcs of E+ as the s3grl_wp_* kernels read them (batch-local
    pointers, a node as its position in its own subgraph): in_ptr / in_nbr / in_dst / in_flag by target node, out_ptr
    / out_nbr / out_arc by source node, `link` the link of every node; num_arcs, max_arcs (host ints)."""

    def __init__(self, split, ids, ids_d, rows, node_ptr, max_nodes, link, arcs, arc_shift, ashift, max_arcs):
        super().__init__(split.subs, ids, ids_d, rows, node_ptr, max_nodes, split.gcn)
        dev = rows.device
        e = int(arcs.numel())
        self.link = link.to(torch.int32)
        shift = ashift[link]
        tail = torch.full((1,), e, dtype=torch.int64, device=dev)
        self.in_ptr = torch.cat([split.in_ptr[rows] - shift, tail])
        self.out_ptr = torch.cat([split.out_ptr[rows] - shift, tail])
        self.in_nbr, self.in_dst, self.in_flag = split.in_nbr[arcs], split.in_dst[arcs], split.in_flag[arcs]
        self.out_nbr, self.out_arc = split.out_nbr[arcs], split.out_arc[arcs] - arc_shift
        self.num_arcs, self.max_arcs = e, int(max_arcs)
        self._c = None

    def in_edge_index(self):
        """[2, e] batch-local (source, target) of every arc of E+ in the kernels' in-order, and the mask [e] that is
        False on the candidate arcs: the reference's (edge_index, edge_mask) of plus_edge / minus_edge."""
        first = self.node_ptr[:-1][self.link.long()]
        tgt = torch.repeat_interleave(torch.arange(self.num_nodes, device=first.device), self.in_ptr.diff(),
                                      output_size=self.num_arcs)
        return torch.stack([self.in_nbr.long() + first[tgt], tgt]), self.in_flag == 0

    def c_struct(self):
        if self._c is None:
            c = N.WpBatch()
            for name in ("node_ptr", "link", "in_ptr", "in_nbr", "in_dst", "in_flag", "out_ptr", "out_nbr", "out_arc"):
                setattr(c, name, N.ptr(getattr(self, name)))
            c.num_links, c.num_nodes, c.num_arcs = self.num_graphs, self.num_nodes, self.num_arcs
            c.max_nodes, c.max_arcs = self.max_nodes, self.max_arcs
            self._c = c
        return C.byref(self._c)


# ---- the two operators ---------------------------------------------------------------------------------------------
class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, batch):
        eng = default_engine(q.device)
        q, k = q.contiguous(), k.contiguous()
        _, heads, hidden = q.shape
        e, dev = batch.num_arcs, q.device
        w, wp, wm = (torch.empty((e, heads), dtype=torch.float32, device=dev) for _ in range(3))
        omega = torch.empty((batch.num_graphs, heads), dtype=torch.float32, device=dev)
        N.check(N.lib().s3grl_wp_attention_forward(eng._ctx, batch.c_struct(), heads, hidden, N.ptr(q), N.ptr(k),
                                                   N.ptr(w), N.ptr(wp), N.ptr(wm), N.ptr(omega)),
                "s3grl_wp_attention_forward")
        ctx.save_for_backward(q, k, w, wp, wm)
        ctx.batch = batch
        return wp, wm, omega

    @staticmethod
    def backward(ctx, gp, gm, gomega):
        q, k, w, wp, wm = ctx.saved_tensors
        eng = default_engine(q.device)
        _, heads, hidden = q.shape
        gp = gp.contiguous() if gp is not None else torch.zeros_like(wp)
        gm = gm.contiguous() if gm is not None else torch.zeros_like(wm)
        gomega = gomega.contiguous() if gomega is not None else torch.zeros((ctx.batch.num_graphs, heads),
                                                                             dtype=torch.float32, device=q.device)
        dw, dq, dk = torch.empty_like(w), torch.empty_like(q), torch.empty_like(k)
        N.check(N.lib().s3grl_wp_attention_backward(eng._ctx, ctx.batch.c_struct(), heads, hidden, N.ptr(q), N.ptr(k),
                                                    N.ptr(w), N.ptr(wp), N.ptr(wm), N.ptr(gp), N.ptr(gm),
                                                    N.ptr(gomega), N.ptr(dw), N.ptr(dq), N.ptr(dk)),
                "s3grl_wp_attention_backward")
        return dq, dk, None


def _check_batch(batch):
    if not isinstance(batch, WalkPoolBatch):
        raise ValueError("batch must come from WalkPoolSplit.batch(...)")
    if batch.max_nodes > N.WP_MAX_NODES:
        raise NotImplementedError(f"a subgraph of {batch.max_nodes} nodes: the walk-pool kernels take at most "
                                  f"{N.WP_MAX_NODES}")


def attention_weights(q, k, batch):
    """(weights_p, weights_m [e, heads], omega [B, heads]) of q, k fp32 [n, heads, hidden] on the GPU over the arcs
    of E+ of `batch` (`WalkPoolSplit.batch`), arcs in the batch's in-order (`batch.in_edge_index()`).  Differentiable
    in q and k."""
    for name, t in (("q", q), ("k", k)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3:
            raise ValueError(f"{name} must be a float32 tensor [n, heads, hidden]")
    if q.shape != k.shape:
        raise ValueError(f"q and k differ in shape: {tuple(q.shape)} and {tuple(k.shape)}")
    if not 1 <= q.shape[1] <= N.WP_MAX_HEADS or not 1 <= q.shape[2] <= N.WP_MAX_HIDDEN:
        raise ValueError(f"heads must be in [1, {N.WP_MAX_HEADS}] and hidden in [1, {N.WP_MAX_HIDDEN}]")
    if not q.is_cuda or not k.is_cuda:
        raise RuntimeError("attention_weights runs on the MI355X only; there is no CPU fallback")
    _check_batch(batch)
    if q.shape[0] != batch.num_nodes:
        raise ValueError(f"q has {q.shape[0]} rows, the batch {batch.num_nodes} nodes")
    return _Attention.apply(q, k, batch)


def _workspace(batch, plan, dev):
    return torch.empty(max(batch.num_graphs * plan["workspace_bytes"] // 4, 4), dtype=torch.float32, device=dev)


class _WalkPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, wp, wm, batch, walk_len, lds_budget):
        eng = default_engine(wp.device)
        wp, wm = wp.contiguous(), wm.contiguous()
        heads = wp.shape[1]
        plan = layout(batch.max_nodes, batch.max_arcs, heads, walk_len, lds_budget)["forward"]
        ws = _workspace(batch, plan, wp.device)
        out = torch.empty((batch.num_graphs, heads, walk_len, WALK_FEATURES), dtype=torch.float32, device=wp.device)
        N.check(N.lib().s3grl_wp_walk_forward(eng._ctx, batch.c_struct(), heads, walk_len, lds_budget, N.ptr(wp),
                                              N.ptr(wm), N.ptr(ws), ws.numel() * 4, N.ptr(out)),
                "s3grl_wp_walk_forward")
        ctx.save_for_backward(wp, wm)
        ctx.batch, ctx.walk_len, ctx.lds_budget = batch, walk_len, lds_budget
        return out

    @staticmethod
    def backward(ctx, gout):
        wp, wm = ctx.saved_tensors
        eng = default_engine(wp.device)
        batch, heads = ctx.batch, wp.shape[1]
        plan = layout(batch.max_nodes, batch.max_arcs, heads, ctx.walk_len, ctx.lds_budget)["backward"]
        ws = _workspace(batch, plan, wp.device)
        gout = gout.contiguous()
        gp, gm = torch.empty_like(wp), torch.empty_like(wm)
        N.check(N.lib().s3grl_wp_walk_backward(eng._ctx, batch.c_struct(), heads, ctx.walk_len, ctx.lds_budget,
                                               N.ptr(wp), N.ptr(wm), N.ptr(gout), N.ptr(ws), ws.numel() * 4,
                                               N.ptr(gp), N.ptr(gm)), "s3grl_wp_walk_backward")
        return gp, gm, None, None, None


def walk_pool(weights_p, weights_m, batch, walk_len, lds_budget=0):
    """[B, heads, walk_len, 5] fp32: for tau = t + 2 the features graphlevel, nodelevel_p, nodelevel_m, linklevel_p,
    linklevel_m of weights_p, weights_m fp32 [e, heads] on the GPU (arcs in the batch's in-order).  lds_budget: bytes of
    LDS a workgroup may use (0 = 80 KiB; 1 keeps every block in an HBM workspace).  Differentiable in both weights."""
    walk_len = _check_walk_len(walk_len)
    for name, t in (("weights_p", weights_p), ("weights_m", weights_m)):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{name} must be a float32 tensor [e, heads]")
    if weights_p.shape != weights_m.shape:
        raise ValueError("weights_p and weights_m differ in shape")
    if not 1 <= weights_p.shape[1] <= N.WP_MAX_HEADS:
        raise ValueError(f"heads must be in [1, {N.WP_MAX_HEADS}]")
    if isinstance(lds_budget, bool) or int(lds_budget) != lds_budget or not 0 <= int(lds_budget) < 2**31:
        raise ValueError("lds_budget must be an integer >= 0")
    if not weights_p.is_cuda or not weights_m.is_cuda:
        raise RuntimeError("walk_pool runs on the MI355X only; there is no CPU fallback")
    _check_batch(batch)
    if weights_p.shape[0] != batch.num_arcs:
        raise ValueError(f"the weights have {weights_p.shape[0]} rows, the batch {batch.num_arcs} arcs")
    return _WalkPool.apply(weights_p, weights_m, batch, walk_len, int(lds_budget))


# ---- the model -----------------------------------------------------------------------------------------------------
class WalkPooling(nn.Module):
    """Reference WalkPooling (model.py:60-219): the attention encoder (lin_key1 / lin_query1 -> leaky_relu 0.2 ->
    dropout 0.5 -> lin_key2 / lin_query2, [n, heads, hidden]) and the walk profile.  forward(x, batch) returns
    [B, heads·(5·walk_len + 1)] with the columns [graphlevel | omega | nodelevel_p | nodelevel_m | linklevel_p |
    linklevel_m], each walk group indexed head·walk_len + t."""

    def __init__(self, in_channels, hidden_channels, heads=1, walk_len=6):
        super().__init__()
        self.hidden_channels, self.heads, self.walk_len = int(hidden_channels), int(heads), _check_walk_len(walk_len)
        self.dropout = 0.5
        self.lin_key1 = nn.Linear(in_channels, hidden_channels)
        self.lin_query1 = nn.Linear(in_channels, hidden_channels)
        self.lin_key2 = nn.Linear(hidden_channels, heads * hidden_channels)
        self.lin_query2 = nn.Linear(hidden_channels, heads * hidden_channels)

    def forward(self, x, batch, lds_budget=0):
        drop = lambda t: F.dropout(t, p=self.dropout, training=self.training)   # noqa: E731
        q = self.lin_key2(drop(F.leaky_relu(self.lin_key1(x), 0.2))).view(-1, self.heads, self.hidden_channels)
        k = self.lin_query2(drop(F.leaky_relu(self.lin_query1(x), 0.2))).view(-1, self.heads, self.hidden_channels)
        wp, wm, omega = attention_weights(q, k, batch)
        walks = walk_pool(wp, wm, batch, self.walk_len, lds_budget)           # [B, heads, walk_len, 5]
        walks = walks.permute(0, 3, 1, 2).reshape(batch.num_graphs, WALK_FEATURES, self.heads * self.walk_len)
        return torch.cat([walks[:, 0], omega, walks[:, 1], walks[:, 2], walks[:, 3], walks[:, 4]], dim=1)


class WalkPoolMLP(nn.Module):
    """Reference MLP (model.py:222-251): BatchNorm1d(L), Linear L -> 20L -> 20L -> 10L -> L with ReLU, dropout 0.5,
    Linear L -> 1, and a sigmoid with MSE."""

    def __init__(self, input_size, MSE=True):
        super().__init__()
        L = int(input_size)
        self.nn = nn.BatchNorm1d(L)
        self.linear1 = nn.Linear(L, L * 20)
        self.linear2 = nn.Linear(L * 20, L * 20)
        self.linear3 = nn.Linear(L * 20, L * 10)
        self.linear4 = nn.Linear(L * 10, L)
        self.linear5 = nn.Linear(L, 1)
        self.MSE, self.dropout = bool(MSE), 0.5

    def forward(self, x):
        x = self.nn(x)
        for lin in (self.linear1, self.linear2, self.linear3, self.linear4):
            x = F.relu(lin(x))
        x = self.linear5(F.dropout(x, p=self.dropout, training=self.training))
        return torch.sigmoid(x) if self.MSE else x


class LinkPredTwin(nn.Module):
    """Reference LinkPred (model.py:13-57) on a `WalkPoolBatch`: optional DRNL embedding beside x, two GCNConv on E+
    with ReLU and dropout 0.5 between them, x_out = [x | conv1 | conv2], WalkPooling, the MLP.  The parameter names
    are the reference's, so a state_dict moves across.  forward(batch) returns [B, 1]."""

    def __init__(self, in_channels, hidden_channels, heads=1, walk_len=6, drnl=False, z_max=100, MSE=True):
        super().__init__()
        self.drnl, self.dropout = bool(drnl), 0.5
        if self.drnl:
            self.z_embedding = nn.Embedding(z_max, hidden_channels)
        self.conv1 = GCNConv(in_channels, hidden_channels)
        self.conv2 = GCNConv(hidden_channels, hidden_channels)
        self.wp = WalkPooling(in_channels + 2 * hidden_channels, hidden_channels, heads, walk_len)
        self.classifier = WalkPoolMLP((5 * self.wp.walk_len + 1) * heads, MSE=MSE)

    def forward(self, batch, lds_budget=0):
        if batch.x is None:
            raise ValueError("the batch has no node features x")
        x = batch.x.to(torch.float32)
        if self.drnl:
            z = self.z_embedding(batch.z)
            if z.dim() == 3:
                z = z.sum(dim=1)
            x = torch.cat([x, z], dim=1)
        h1 = self.conv1(x, batch)
        h2 = self.conv2(F.dropout(h1.relu(), p=self.dropout, training=self.training), batch)
        return self.classifier(self.wp(torch.cat([x, h1, h2], dim=1), batch, lds_budget))


# ---- one Table 2 row -----------------------------------------------------------------------------------------------
def _epoch_order(n, seed, epoch):
    return np.random.default_rng([int(seed) & 0xffffffff, int(epoch)]).permutation(n)


def run_walkpool(split, x=None, *, num_hops=2, max_nodes_per_hop=None, walk_len=7, heads=2, hidden=32, drnl=False,
                 MSE=False, lr=5e-5, weight_decay=0, batch_size=32, epochs=50, embedding_dim=32, seed=1, device=None):
    """The WalkPool row from a `workloads.Split` (reference main.py:176-262): the train graph is split.A, the six
    link lists are labelled 1 / 0; x = None is ones of width embedding_dim.  Adam (lr, weight_decay), BCE with logits
    (MSE on the sigmoid with MSE), batches of batch_size links in a fresh order every epoch, validation and test
    AUC / AP on the device after every epoch.  Returns {'history': one dict per epoch ('epoch', 'train_loss',
    'val_loss', 'val_auc', 'val_ap', 'test_auc', 'test_ap'), 'best_val_auc' / 'best_val_loss': {'epoch', 'test_auc',
    'test_ap'} picked at the first best epoch, 'scores': {'valid', 'test'} of the last epoch with 'labels' beside
    them (device tensors), 'model'}.  One deviation: 'val_loss' is the mean over the validation links; the reference
    keeps the loss of the last batch of a shuffled loader.  NotImplementedError for a directed graph (split.A not
    symmetric)."""
    from .metrics import LinkMetrics
    from .seal import enclosing_subgraphs

    A = split.A
    if (A != A.T).nnz:
        raise NotImplementedError("WalkPool on a directed graph (split.A is not symmetric): the reference has none")
    walk_len = _check_walk_len(walk_len)
    if int(batch_size) < 1 or int(epochs) < 1 or not lr > 0:
        raise ValueError("need batch_size >= 1, epochs >= 1 and lr > 0")
    n = int(split.num_nodes)
    if x is None:
        x = torch.ones((n, int(embedding_dim)), dtype=torch.float32)
    x = torch.as_tensor(x, dtype=torch.float32)
    if x.dim() != 2 or x.shape[0] != n:
        raise ValueError(f"x must be [{n}, F]")
    eng = default_engine(device)
    dev = eng.device
    torch.manual_seed(seed)                      # initial parameters and the dropout masks

    lists, labels = {}, {}
    for name in ("train", "valid", "test"):
        pos, neg = (np.asarray(a, dtype=np.int64) for a in split.links[name])
        links = torch.from_numpy(np.concatenate([pos, neg], axis=1))
        subs = enclosing_subgraphs(links, split.A, x, 0, num_hops, node_label="drnl" if drnl else "zo",
                                   max_nodes_per_hop=max_nodes_per_hop, seed=seed, engine=eng)
        lists[name] = WalkPoolSplit(subs)
        labels[name] = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(dev)
    z_max = 100
    if drnl:
        z_max = max(z_max, 1 + max(int(w.subs.subs.z.max()) for w in lists.values() if len(w)))
    # with DRNL the label embedding (hidden wide) stands beside x (reference main.py:169-170)
    model = LinkPredTwin(x.shape[1] + (hidden if drnl else 0), hidden, heads, walk_len, drnl=drnl, z_max=z_max,
                         MSE=MSE).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)
    metrics = LinkMetrics(dev)

    def loss_of(out, y, reduction="mean"):
        if MSE:
            return F.mse_loss(out.view(-1), y, reduction=reduction)
        return F.binary_cross_entropy_with_logits(out.view(-1), y, reduction=reduction)

    def evaluate(name):
        wps, y = lists[name], labels[name]
        scores = torch.empty(len(wps), dtype=torch.float32, device=dev)
        with torch.no_grad():
            for a in range(0, len(wps), batch_size):
                ids = np.arange(a, min(a + batch_size, len(wps)))
                scores[a:a + ids.size] = model(wps.batch(ids)).view(-1)
            loss = loss_of(scores, y)
        r = metrics.ranked(scores, y)
        return scores, float(loss), r["AUC"], r["AP"]

    history, scores = [], {}
    n_train = len(lists["train"])
    for epoch in range(1, int(epochs) + 1):
        model.train()
        order = _epoch_order(n_train, seed, epoch)
        total, seen = torch.zeros((), dtype=torch.float32, device=dev), 0
        for a in range(0, n_train, batch_size):
            ids = order[a:a + batch_size]
            if ids.size < 2:                     # BatchNorm in training mode needs two rows
                continue
            opt.zero_grad(set_to_none=True)
            out = model(lists["train"].batch(ids))
            y = labels["train"][torch.from_numpy(ids).to(dev)]
            loss = loss_of(out, y)
            loss.backward()
            opt.step()
            total += loss.detach() * ids.size
            seen += ids.size
        model.eval()
        scores["valid"], val_loss, val_auc, val_ap = evaluate("valid")
        scores["test"], _, test_auc, test_ap = evaluate("test")
        history.append({"epoch": epoch, "train_loss": float(total) / max(seen, 1), "val_loss": val_loss,
                        "val_auc": val_auc, "val_ap": val_ap, "test_auc": test_auc, "test_ap": test_ap})
    by_auc = max(history, key=lambda h: (h["val_auc"], -h["epoch"]))
    by_loss = min(history, key=lambda h: (h["val_loss"], h["epoch"]))
    pick = lambda h: {"epoch": h["epoch"], "test_auc": h["test_auc"], "test_ap": h["test_ap"]}   # noqa: E731
    return {"history": history, "best_val_auc": pick(by_auc), "best_val_loss": pick(by_loss), "scores": scores,
            "labels": {k: labels[k] for k in ("valid", "test")}, "model": model}
