"""Labelled enclosing subgraphs for the SEAL baselines (reference utils.py:556-573: `k_hop_subgraph` then
`construct_pyg_graph` with a node-labelling trick, per link), computed for the whole link list at once by
the engine (s3grl_subgraphs_* in include/s3grl.h, kernels in csrc/s3grl_seal.hip).

    subs = enclosing_subgraphs(link_index, A, x, y, num_hops, node_label="drnl")
    subs[i]            # Data(x, edge_index, edge_weight, y, z, node_id, num_nodes) of link i
    subs.collate_pyg() # one batch of all links: what the reference's DGCNN / GCN consume

Everything stays on the device.  Importing this module does no work.
"""
from __future__ import annotations

import ctypes as C
from collections.abc import Sequence as _Sequence
from dataclasses import dataclass

import numpy as np
import torch

from . import _native as N

try:  # PyG present: real Data objects
    from torch_geometric.data import Data as _PygData  # type: ignore
except Exception:  # PyG absent: attribute / item compatible stand-in
    _PygData = None


class SubgraphData:
    """Minimal stand-in for torch_geometric.data.Data: attribute and item access, `keys()`, `to(device)`."""

    def __init__(self, **kw):
        self.__dict__["_store"] = dict(kw)

    def __getattr__(self, k):
        try:
            return self.__dict__["_store"][k]
        except KeyError:
            raise AttributeError(k)

    def __getitem__(self, k):
        return self._store[k]

    def __contains__(self, k):
        return k in self._store

    def keys(self):
        return list(self._store.keys())

    def to(self, device):
        return SubgraphData(**{k: (v.to(device) if torch.is_tensor(v) else v) for k, v in self._store.items()})

    def __repr__(self):
        parts = [f"{k}={list(v.shape) if torch.is_tensor(v) else v}" for k, v in self._store.items()]
        return "SubgraphData(" + ", ".join(parts) + ")"


def _make_data(**kw):
    return _PygData(**kw) if _PygData is not None else SubgraphData(**kw)


@dataclass
class LabelledSubgraphs:
    """The engine's output, device tensors: link l owns nodes[node_ptr[l]:node_ptr[l+1]] and
    src / dst / weight[edge_ptr[l]:edge_ptr[l+1]] (local ids into its own node list)."""
    node_ptr: torch.Tensor   # int64 [L+1]
    nodes: torch.Tensor      # int32 [Σn] global ids: src, dst, then hop-major, ascending id inside a hop
    dists: torch.Tensor      # int8 [Σn]
    edge_ptr: torch.Tensor   # int64 [L+1]
    src: torch.Tensor        # int32 [Σe]
    dst: torch.Tensor        # int32 [Σe]
    weight: torch.Tensor     # fp32 [Σe]
    z: torch.Tensor          # int32 [Σn] or [Σn, 2] (de, de+)


def label_code(node_label):
    if not isinstance(node_label, str):
        raise ValueError("node_label must be a string")
    return N.LABELS.get(node_label, N.LABEL_ZEROS)


def labelled_subgraphs(engine, graph, links, *, num_hops, node_label="drnl", values=None, ratio_per_hop=1.0,
                       max_nodes_per_hop=None, seed=0, lds_budget=0):
    """Engine-level call.  graph: `Engine.graph(...)`; links int64 [L, 2] on the device (`Engine.links`);
    values fp32 [nnz] on the device aligned with the graph's CSR entries, or None for ones.  lds_budget: bytes
    of LDS a link may use (0 = the default; 1 sends every link to the HBM flavour)."""
    code = label_code(node_label)
    cfg = _cfg(num_hops, ratio_per_hop, max_nodes_per_hop, seed, lds_budget)
    if values is not None:
        assert values.is_cuda and values.dtype == torch.float32 and values.numel() == graph.nnz
    lib = N.lib()
    h = C.c_void_p()
    L = int(links.shape[0])
    N.check(lib.s3grl_subgraphs_create(engine._ctx, graph._h, N.ptr(values), N.ptr(links), L, C.byref(cfg), code,
                                       C.byref(h)), "s3grl_subgraphs_create")
    try:
        cnt = (C.c_int64 * 4)()
        N.check(lib.s3grl_subgraphs_counts(h, cnt), "s3grl_subgraphs_counts")
        n, e, zw = int(cnt[1]), int(cnt[2]), int(cnt[3])
        dev = engine.device
        out = LabelledSubgraphs(
            node_ptr=torch.empty(L + 1, dtype=torch.int64, device=dev),
            nodes=torch.empty(n, dtype=torch.int32, device=dev),
            dists=torch.empty(n, dtype=torch.int8, device=dev),
            edge_ptr=torch.empty(L + 1, dtype=torch.int64, device=dev),
            src=torch.empty(e, dtype=torch.int32, device=dev),
            dst=torch.empty(e, dtype=torch.int32, device=dev),
            weight=torch.empty(e, dtype=torch.float32, device=dev),
            z=torch.empty((n, 2) if zw == 2 else (n,), dtype=torch.int32, device=dev))
        N.check(lib.s3grl_subgraphs_export(h, N.ptr(out.node_ptr), N.ptr(out.nodes), N.ptr(out.dists),
                                           N.ptr(out.edge_ptr), N.ptr(out.src), N.ptr(out.dst), N.ptr(out.weight),
                                           N.ptr(out.z)), "s3grl_subgraphs_export")
    finally:
        lib.s3grl_subgraphs_destroy(h)
    return out


def _cfg(num_hops, ratio_per_hop, max_nodes_per_hop, seed, lds_budget):
    cfg = N.SubgraphCfg()
    if isinstance(num_hops, bool) or int(num_hops) != num_hops or not 1 <= int(num_hops) <= 30:
        raise ValueError("num_hops must be an integer in [1, 30]")
    cfg.num_hops = int(num_hops)
    cfg.seed = int(seed) & 0xffffffff
    if ratio_per_hop is None or not float(ratio_per_hop) > 0.0:
        raise ValueError("ratio_per_hop must be > 0")
    cfg.ratio_per_hop = min(float(ratio_per_hop), 1.0)
    if max_nodes_per_hop is not None:
        if int(max_nodes_per_hop) < 1:
            raise ValueError("max_nodes_per_hop must be >= 1 (or None)")
        cfg.max_nodes_per_hop = int(max_nodes_per_hop)
    if not 0 <= int(lds_budget) < 2**31:
        raise ValueError("lds_budget must be >= 0")
    cfg.lds_budget = int(lds_budget)
    return cfg


def _check_links(link_index, num_nodes):
    li = torch.as_tensor(link_index)
    if li.dim() != 2 or li.shape[0] != 2:
        raise ValueError("link_index must be [2, L]")
    if li.dtype.is_floating_point or li.dtype == torch.bool:
        raise ValueError("link_index must hold integer node ids")
    if not li.is_cuda and li.numel():
        if int(li.min()) < 0 or int(li.max()) >= num_nodes:
            raise ValueError("a link endpoint is outside [0, num_nodes)")
        if bool((li[0] == li[1]).any()):
            raise ValueError("a link has src == dst")
    return li


class SubgraphList(_Sequence):
    """The labelled subgraphs of a link list: item i is the reference's `construct_pyg_graph` Data of link i
    (x, edge_index, edge_weight, y, z, node_id, num_nodes), built on access from the device arrays."""

    def __init__(self, subs: LabelledSubgraphs, x, y, weight_dtype, node_label):
        self.subs = subs
        self.x = x                        # device [N, F] or None
        self.y = y
        self.weight_dtype = weight_dtype
        self.node_label = node_label
        self._node_ptr = subs.node_ptr.cpu().tolist()
        self._edge_ptr = subs.edge_ptr.cpu().tolist()
        self._counts = np.diff(np.asarray(self._node_ptr, dtype=np.int64))
        self._gcn = {}                    # use_edge_weight -> propagate.GcnSplit, built on the first batch
        self._nbr = None                  # propagate.NbrSplit (the raw-edge operator), built on first use

    def __len__(self):
        return len(self._node_ptr) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        s = self.subs
        a, b = self._node_ptr[i], self._node_ptr[i + 1]
        c, d = self._edge_ptr[i], self._edge_ptr[i + 1]
        node_id = s.nodes[a:b].long()
        edge_index = torch.stack([s.src[c:d], s.dst[c:d]], 0).long()
        return _make_data(x=self.x[node_id] if self.x is not None else None, edge_index=edge_index,
                          edge_weight=s.weight[c:d].to(self.weight_dtype), y=torch.tensor([self.y]),
                          z=s.z[a:b].long(), node_id=node_id, num_nodes=b - a)

    def node_counts(self):
        """Nodes of every subgraph, host int64 [L] (no device read)."""
        return self._counts.copy()

    def gcn_split(self, use_edge_weight=False):
        """The GCN operator of the whole split (`propagate.GcnSplit`), built once and kept."""
        key = bool(use_edge_weight)
        if key not in self._gcn:
            from .propagate import GcnSplit

            self._gcn[key] = GcnSplit(self, use_edge_weight=key)
        return self._gcn[key]

    def nbr_split(self):
        """The raw-edge operator of the whole split (`propagate.NbrSplit`, for SAGE and GIN), built once and kept."""
        if self._nbr is None:
            from .propagate import NbrSplit

            self._nbr = NbrSplit(self)
        return self._nbr

    def batch(self, link_ids, use_edge_weight=False):
        """The device batch of the links `link_ids` (host integers, in that order) for `seal_nn.DGCNNTwin` /
        `GCNTwin`: their subgraphs back to back, x and z gathered for these nodes only.  Sizes come from the
        host copies of node_ptr / edge_ptr, so nothing waits for the device.  use_edge_weight: the GCN operator
        normalises with the edge weights (the reference's --use_edge_weight) instead of ones."""
        ids = np.asarray(link_ids, dtype=np.int64).reshape(-1)
        L = len(self)
        if ids.size and (ids.min() < 0 or ids.max() >= L):
            raise IndexError("link id outside the list")
        counts = self._counts[ids]
        local = np.zeros(ids.size + 1, dtype=np.int64)
        np.cumsum(counts, out=local[1:])
        n = int(local[-1])
        dev = self.subs.node_ptr.device
        B = ids.size
        both = _to_device(np.concatenate([ids, local, counts]), dev)      # one host -> device copy
        ids_d, ptr_d, cnt_d = both[:B], both[B:2 * B + 1], both[2 * B + 1:]
        rows = torch.repeat_interleave(self.subs.node_ptr[ids_d] - ptr_d[:-1], cnt_d, output_size=n) + \
            torch.arange(n, device=dev)
        return SealBatch(self, ids, ids_d, rows, ptr_d, int(counts.max()) if ids.size else 0,
                         self.gcn_split(use_edge_weight))

    def collate_pyg(self):
        """All links as one batch: x gathered from node_id, edge_index offset by each link's first node,
        `batch` (link of every node), z, y [L], node_id, ptr (= node_ptr)."""
        s = self.subs
        L = len(self)
        dev = s.node_ptr.device
        links = torch.arange(L, device=dev)
        batch = torch.repeat_interleave(links, s.node_ptr.diff())
        edge_link = torch.repeat_interleave(links, s.edge_ptr.diff())
        first = s.node_ptr[:-1][edge_link]
        edge_index = torch.stack([s.src.long() + first, s.dst.long() + first], 0)
        node_id = s.nodes.long()
        return _make_data(x=self.x[node_id] if self.x is not None else None, edge_index=edge_index,
                          edge_weight=s.weight.to(self.weight_dtype), y=torch.full((L,), self.y, device=dev),
                          z=s.z.long(), node_id=node_id, batch=batch, ptr=s.node_ptr.clone(),
                          num_nodes=int(s.nodes.numel()))


def enclosing_subgraphs(link_index, A, x, y, num_hops, node_label="drnl", ratio_per_hop=1.0,
                        max_nodes_per_hop=None, directed=False, A_csc=None, *, seed=0, engine=None, lds_budget=0):
    """The reference's SEAL loop (utils.py:556-573) in one call, with its argument order: link_index [2, L],
    A the scipy CSR train graph (values become edge_weight, in A's dtype), x [N, F] or None, y the label of
    every link.  Sampling (ratio_per_hop < 1, max_nodes_per_hop) draws with the engine's keyed generator
    (`seed`), like a PoS plan.  Returns a `SubgraphList` of device tensors."""
    import scipy.sparse as ssp

    if not ssp.issparse(A) or A.shape[0] != A.shape[1]:
        raise ValueError("A must be a square scipy sparse matrix")
    A = ssp.csr_matrix(A)
    if not A.has_canonical_format:
        A = A.copy()
        A.sum_duplicates()
    num_nodes = A.shape[0]
    li = _check_links(link_index, num_nodes)
    label_code(node_label)                                                 # argument checks before any GPU work
    _cfg(num_hops, ratio_per_hop, max_nodes_per_hop, seed, lds_budget)
    if x is not None:
        x = torch.as_tensor(x)
        if x.dim() < 1 or x.shape[0] != num_nodes:
            raise ValueError("x must have one row per node of A")
    weight_dtype = torch.from_numpy(np.zeros(0, dtype=A.dtype)).dtype
    from .engine import default_engine

    eng = engine if engine is not None else default_engine()
    g = eng.graph(A, directed=directed, A_csc=A_csc if directed else None)
    try:
        values = None
        if A.nnz and not (A.data == 1).all():
            values = torch.as_tensor(np.asarray(A.data, dtype=np.float32)).to(eng.device)
        subs = labelled_subgraphs(eng, g, eng.links(li), num_hops=num_hops, node_label=node_label,
                                  values=values, ratio_per_hop=ratio_per_hop, max_nodes_per_hop=max_nodes_per_hop,
                                  seed=seed, lds_budget=lds_budget)
    finally:
        g.close()
    xd = x.to(eng.device) if x is not None else None
    return SubgraphList(subs, xd, y, weight_dtype, node_label)


def _to_device(a, dev):
    """Host int64 array -> device, asynchronously (pinned staging; nothing waits for the device)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64))
    if dev.type == "cuda":
        t = t.pin_memory()
    return t.to(dev, non_blocking=True)


class SealBatch:
    """A mini-batch of `SubgraphList.batch`: the subgraphs of `link_ids` back to back on the device.

    x [n, F] or None (rows of the list's x by global node id), z [n] or [n, 2] (int64), node_ptr [B+1] (local),
    rows [n] (the split position of every batch node: an index into subs.nodes / subs.z), gcn (the split's GCN operator), link_ids (host) / link_ids_device, num_graphs, num_nodes, max_nodes
    (host ints).  edge_index [2, e] (batch-local, grouped by subgraph) and edge_weight [e] are built on access."""

    def __init__(self, subs, ids, ids_d, rows, node_ptr, max_nodes, gcn):
        self._subs = subs
        self.link_ids, self.link_ids_device = ids, ids_d
        self.rows, self.node_ptr, self.gcn = rows, node_ptr, gcn
        self.num_graphs, self.num_nodes, self.max_nodes = int(ids.size), int(rows.numel()), int(max_nodes)
        self.x = subs.x[subs.subs.nodes[rows].long()] if subs.x is not None else None   # by global node id
        self.z = subs.subs.z[rows].long()
        self._edges = None

    def _edge_rows(self):
        if self._edges is None:
            sl, s = self._subs, self._subs.subs
            ep = np.asarray(sl._edge_ptr, dtype=np.int64)
            ecnt = ep[self.link_ids + 1] - ep[self.link_ids]
            e = int(ecnt.sum())
            dev = self.rows.device
            cnt_d = _to_device(ecnt, dev)
            elocal = torch.zeros(self.num_graphs + 1, dtype=torch.int64, device=dev)
            elocal[1:] = torch.cumsum(cnt_d, 0)
            eidx = torch.repeat_interleave(s.edge_ptr[self.link_ids_device] - elocal[:-1], cnt_d, output_size=e) + \
                torch.arange(e, device=dev)
            first = torch.repeat_interleave(self.node_ptr[:-1], cnt_d, output_size=e)
            self._edges = (eidx, first)
        return self._edges

    @property
    def nbr(self):
        """The split's raw-edge operator (`propagate.NbrSplit`), built on the first access of any batch of the list."""
        return self._subs.nbr_split()

    @property
    def edge_index(self):
        eidx, first = self._edge_rows()
        s = self._subs.subs
        return torch.stack([s.src[eidx].long() + first, s.dst[eidx].long() + first], 0)

    @property
    def edge_weight(self):
        eidx, _ = self._edge_rows()
        return self._subs.subs.weight[eidx].to(self._subs.weight_dtype)
