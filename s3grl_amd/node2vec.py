"""node2vec pretraining for `init_features: "n2v"` (reference n2v_prep.py, sgrl_link_pred.py:966-971): a twin of PyG
`Node2Vec(..., p=1, q=1, sparse=True)` trained by `torch.optim.SparseAdam`, whose every step runs as HIP kernels
behind the C ABI (s3grl_skipgram_*, csrc/s3grl_node2vec.hip).

    emb = node_2_vec_pretrain("USAir", edge_index, num_nodes, 16, seed, device, 50)      # the reference's call
    n2v = Node2Vec(edge_index, num_nodes, 16, seed=0); losses = n2v.fit(50); x = n2v.embedding()

Same algorithm as PyG 2.0.x: per epoch a permutation of range(N) in batches; per batch `walks_per_node` uniform
walks from every start and as many rows of uniform negatives, cut into `context_size` windows window-major; the
loss `-log(sigmoid(<h0, hi>) + EPS)` / `-log(1 - sigmoid(...) + EPS)`, each mean over its own dots; SparseAdam on
the coalesced rows.  The random draws come from the engine's counter-based generator keyed by (seed, epoch, step,
position), not from torch's and torch_cluster's streams, so embeddings are NOT bit-equal to PyG's: same algorithm,
same distributions, same update given the same windows.  Two runs with one seed are bit-identical.  GPU only; no
CPU fallback.  Configurations no reference run uses raise NotImplementedError: p != 1, q != 1, sparse=False, an
optimiser other than SparseAdam.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np
import torch

from . import _native as N

MAX_DIM = 1 << 14


def _check_unused(p, q, sparse):
    if p != 1 or q != 1:
        raise NotImplementedError("node2vec with p != 1 or q != 1: no reference config uses it")
    if not sparse:
        raise NotImplementedError("node2vec with sparse=False: the reference trains with sparse=True (SparseAdam)")


def windows_per_walk(walk_length, context_size):
    """PyG's `num_walks_per_rw = 1 + walk_length + 1 - context_size`."""
    return walk_length + 2 - context_size


def csr_of(edge_index, num_nodes):
    """edge_index [2, E] exactly as given (rows = sources, nothing made symmetric, duplicates kept) ->
    (indptr int64 [N+1], indices int32 [E]) grouped by source, in the given order inside a row."""
    ei = np.asarray(edge_index.cpu() if isinstance(edge_index, torch.Tensor) else edge_index)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, E], got {tuple(ei.shape)}")
    ei = ei.astype(np.int64, copy=False)
    if ei.size and (ei.min() < 0 or ei.max() >= num_nodes):
        raise ValueError("edge_index holds a node outside [0, num_nodes)")
    order = np.argsort(ei[0], kind="stable")
    indptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(ei[0], minlength=num_nodes), out=indptr[1:])
    return indptr, ei[1][order].astype(np.int32)


class Node2Vec:
    """PyG `Node2Vec` twin (p = q = 1, sparse=True) with its SparseAdam state on the device."""

    def __init__(self, edge_index, num_nodes, embedding_dim, walk_length=20, context_size=10, walks_per_node=10,
                 num_negative_samples=1, p=1, q=1, sparse=True, seed=0, device=None, init=None):
        _check_unused(p, q, sparse)
        num_nodes, dim = int(num_nodes), int(embedding_dim)
        if num_nodes < 1 or num_nodes >= 1 << 31:
            raise ValueError(f"num_nodes must be in [1, 2^31), got {num_nodes}")
        if not 1 <= dim <= MAX_DIM:
            raise ValueError(f"embedding_dim must be in [1, {MAX_DIM}], got {dim}")
        if context_size < 2:
            raise ValueError("context_size must be at least 2 (a window needs one context node)")
        if walk_length < context_size:
            raise ValueError("walk_length must be at least context_size (PyG asserts it)")
        if walks_per_node < 1 or num_negative_samples < 1:
            raise ValueError("walks_per_node and num_negative_samples must be at least 1")
        if init is not None and tuple(init.shape) != (num_nodes, dim):
            raise ValueError(f"init must be [{num_nodes}, {dim}], got {tuple(init.shape)}")
        indptr, indices = csr_of(edge_index, num_nodes)
        from .engine import default_engine

        self.engine = default_engine(device)
        dev = self.engine.device
        self.num_nodes, self.embedding_dim = num_nodes, dim
        self.walk_length, self.context_size = int(walk_length), int(context_size)
        self.walks_per_node, self.num_negative_samples = int(walks_per_node), int(num_negative_samples)
        self.seed = int(seed)
        self.epochs_done = 0
        cfg = N.SkipgramCfg(dim, self.walk_length, self.context_size, self.walks_per_node, self.num_negative_samples,
                            self.seed & 0xffffffff, 1.0, 1.0)
        ip = torch.as_tensor(indptr).to(dev)
        ix = torch.as_tensor(indices).to(dev)
        x0 = None if init is None else torch.as_tensor(init).to(device=dev, dtype=torch.float32).contiguous()
        h = C.c_void_p()
        N.check(N.lib().s3grl_skipgram_create(self.engine._ctx, num_nodes, N.ptr(ip), N.ptr(ix), int(ix.numel()),
                                              C.byref(cfg), N.ptr(x0), C.byref(h)), "s3grl_skipgram_create")
        self._h = h
        self.engine._children.add(self)   # the engine closes it before its context goes

    # -- training ---------------------------------------------------------------------------------------------
    def steps_per_epoch(self, batch_size=32):
        return -(-self.num_nodes // int(batch_size))

    def fit(self, epochs, batch_size=32, lr=0.01, optimizer="SparseAdam"):
        """`epochs` passes of `loader(batch_size, shuffle=True)` with SparseAdam(lr); returns the per-epoch loss sums
        (the reference's `total_loss`).  The step losses stay on the device until the end: no sync per step."""
        if optimizer != "SparseAdam":
            raise NotImplementedError("node2vec trains with torch.optim.SparseAdam only (reference n2v_prep.py)")
        epochs, batch_size, lr = int(epochs), int(batch_size), float(lr)
        if epochs < 0 or batch_size < 1 or not lr > 0:
            raise ValueError("need epochs >= 0, batch_size >= 1 and lr > 0")
        self._alive()
        steps = self.steps_per_epoch(batch_size)
        losses = torch.empty((epochs, steps), dtype=torch.float32, device=self.engine.device)
        L = N.lib()
        for e in range(epochs):
            N.check(L.s3grl_skipgram_epoch(self._h, self.epochs_done, batch_size, lr, N.ptr(losses[e])),
                    "s3grl_skipgram_epoch")
            self.epochs_done += 1
        return [float(x) for x in losses.cpu().double().sum(dim=1)]

    def windows(self, epoch, step, batch_size=32):
        """The (pos, neg) windows the engine draws at (epoch, step): int64 device tensors [W·B·walks_per_node, C]
        and [W·B·walks_per_node·num_negative_samples, C], window-index-major (PyG's pos_sample / neg_sample)."""
        self._alive()
        B = min(int(batch_size), self.num_nodes - int(step) * int(batch_size))
        if B < 1 or epoch < 0 or step < 0:
            raise ValueError(f"no step {step} of batch size {batch_size} over {self.num_nodes} nodes")
        rows = windows_per_walk(self.walk_length, self.context_size) * B * self.walks_per_node
        dev = self.engine.device
        pos = torch.empty((rows, self.context_size), dtype=torch.int32, device=dev)
        neg = torch.empty((rows * self.num_negative_samples, self.context_size), dtype=torch.int32, device=dev)
        N.check(N.lib().s3grl_skipgram_export_windows(self._h, int(epoch), int(step), int(batch_size), N.ptr(pos),
                                                      N.ptr(neg)), "s3grl_skipgram_export_windows")
        return pos.long(), neg.long()

    def step(self, pos, neg, lr=0.01):
        """One SparseAdam step on the given windows ([P, C] and [Q, C] node ids); returns the step's loss."""
        self._alive()
        dev = self.engine.device
        pos = torch.as_tensor(pos).to(device=dev, dtype=torch.int32).contiguous()
        neg = torch.as_tensor(neg).to(device=dev, dtype=torch.int32).contiguous()
        C_ = self.context_size
        if pos.dim() != 2 or neg.dim() != 2 or pos.shape[1] != C_ or neg.shape[1] != C_ or not pos.shape[0] \
                or not neg.shape[0]:
            raise ValueError(f"windows must be non-empty [*, {C_}] tensors")
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        N.check(N.lib().s3grl_skipgram_step_windows(self._h, N.ptr(pos), pos.shape[0], N.ptr(neg), neg.shape[0],
                                                    float(lr), N.ptr(loss)), "s3grl_skipgram_step_windows")
        return float(loss.item())

    # -- state ------------------------------------------------------------------------------------------------
    def state(self):
        """dict(weight, exp_avg, exp_avg_sq: fp32 [N, D] device copies, step: SparseAdam's step count)."""
        self._alive()
        dev, shape = self.engine.device, (self.num_nodes, self.embedding_dim)
        w, m, v = (torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3))
        steps = C.c_int64()
        N.check(N.lib().s3grl_skipgram_state(self._h, N.ptr(w), N.ptr(m), N.ptr(v), C.byref(steps)),
                "s3grl_skipgram_state")
        return {"weight": w, "exp_avg": m, "exp_avg_sq": v, "step": int(steps.value)}

    def embedding(self):
        """`Node2Vec.forward()` = embedding.weight: fp32 [N, D] on the device (a copy)."""
        return self.state()["weight"]

    def _table(self):
        """The live embedding.weight on the device as a `linkclf.TableRef`: its address, no copy.  For consumers that
        work on the engine's stream while the trainer is open; everyone else takes `embedding()`."""
        from .linkclf import TableRef

        self._alive()
        p = C.c_void_p()
        N.check(N.lib().s3grl_skipgram_weight(self._h, C.byref(p)), "s3grl_skipgram_weight")
        return TableRef(p.value, self.num_nodes, self.embedding_dim, self)

    def _alive(self):
        if getattr(self, "_h", None) is None:
            raise RuntimeError("Node2Vec is closed")

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and self.engine._ctx:   # the trainer works on the context's stream
            N.lib().s3grl_skipgram_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def node_2_vec_pretrain(dataset, edge_index, num_nodes, emb_dim, seed, device, epochs, hypertuning=False,
                        extra_identifier='', cache=False):
    """Reference n2v_prep.node_2_vec_pretrain: walk_length 20, context_size 10, walks_per_node 10, one negative,
    loader(batch_size=32, shuffle=True), SparseAdam(lr=0.01); returns embedding.weight as a detached fp32 CPU
    tensor [N, emb_dim].  cache=True reads / writes Emb/{dataset}_{emb_dim}_seed{seed}_{extra_identifier}.pt (under
    the home directory when hypertuning), as the reference does."""
    emb_folder = f"{Path.home()}/Emb" if hypertuning else "Emb"
    path = f"{emb_folder}/{dataset}_{emb_dim}_seed{seed}_{extra_identifier}.pt"
    if cache and os.path.exists(path):
        return torch.load(path, map_location=torch.device("cpu")).detach()
    if device is not None and torch.device(device).type == "cpu":
        raise RuntimeError("node2vec pretraining needs a HIP device (MI355X); there is no CPU fallback")
    n2v = Node2Vec(edge_index, num_nodes, emb_dim, walk_length=20, context_size=10, walks_per_node=10,
                   num_negative_samples=1, p=1, q=1, sparse=True, seed=seed, device=device)
    n2v.fit(epochs, batch_size=32, lr=0.01)
    out = n2v.embedding().cpu().clone().detach()
    n2v.close()
    if cache:
        os.makedirs(emb_folder, exist_ok=True)
        torch.save(out, path)
    return out
