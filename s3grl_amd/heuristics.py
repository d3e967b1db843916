"""Classic link heuristics of the reference's `--use_heuristic` branch (sgrl_link_pred.py:1049-1090, utils.py:681-742):
common neighbours (CN), Adamic-Adar (AA) and personalised PageRank (PPR), scored by HIP kernels behind the C ABI
(s3grl_heuristics_*, csrc/s3grl_heuristics.hip), plus the AUC / AP evaluation of that branch.

    h = Heuristics(split.A)                   # the graph on the device, prepared once
    cn, aa, ppr = h.cn(links), h.aa(links), h.ppr(links)     # fp32 device tensors, one score per link
    scores, edge_index = PPR(A, edge_index)   # the reference's signature: CPU tensors, links ordered by source
    results = run_heuristic(split, "PPR")     # {'AUC': (val, test), 'AP': (val, test)}

`A` is the reference's scipy CSR of `data.edge_index` (values: edge_weight, or int64 ones).  It is taken with
duplicates summed, explicit zeros dropped and rows sorted, and its values as fp64.

- CN: Σ_k A[s,k]·A[d,k]; AA: Σ_k A[s,k]·(A[d,k]·w_k), w_k = 1/ln(column sum k) in fp64, ±inf -> 0 (a column sum
  of 1), -0.0 for a column sum of 0, negative for a column sum in (0, 1), NaN for a negative column sum, as the
  reference has them.  A NaN weight at any key of row d makes AA(s, d) NaN whatever s is: the reference's sparse
  `A[s].multiply(A_[d])` keeps 0·NaN for the entries that row s lacks.  Both summed in fp64 and returned as fp32:
  with integer weights CN is exact.
- PPR: fast_pagerank 0.0.4 `pagerank_power(A, p, personalize=e_s, tol, max_iter)`: r = A.sum(1),
  W = p·Aᵀ·diag(1/r), z = ((1-p)·[r≠0] + [r=0]) / n, x = n·e_s; while ‖x − x_old‖₂ > tol (on the unnormalised x)
  and fewer than max_iter iterations: x = W·x + n·e_s·(zᵀ·x).  The score of a link is x[d] / Σx.  In fp64, with a
  stop per source; each distinct source is solved once per call, however many links share it.

Four more indices, which the reference does not have (DESIGN.md §23 is their specification), follow the same
conventions.  With r the row sums, c the column sums and deg the stored entries of a row:

    ra, jac, pa, katz = h.ra(links), h.jaccard(links), h.pa(links), h.katz(links, beta=0.005, max_len=3)
    scores, edge_index = Katz(A, edge_index)  # CPU tensors in the given order; likewise RA, Jaccard and PA

- RA: Σ_k A[s,k]·(A[d,k]·v_k), v_k = 1/c_k and 0 where c_k = 0.  PA: r_s·r_d.
- JACCARD: structural, |keys(s) ∩ keys(d)| / (deg(s) + deg(d) − |∩|), 0 when that is 0.
- KATZ: Σ_{l=1..max_len} β^l·(A^l)[s,d] by Horner's rule on Aᵀ, x_l = β·Aᵀ·(x_{l−1} + e_s) from x_0 = 0, in fp64;
  each distinct source is solved once per call.  β finite and 1 <= max_len <= 64, else ValueError.

GPU only; there is no CPU fallback.  Node ids outside [0, N) raise ValueError before any GPU work.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as ssp
import torch

from . import _native as N

KIND = {"CN": 0, "AA": 1, "RA": 2, "JACCARD": 3, "PA": 4}
NAMES = ("CN", "AA", "PPR", "RA", "JACCARD", "PA", "KATZ")
KATZ_MAX_LEN = 64


def canonical_csr(A):
    """The graph as the kernels take it: square CSR, duplicates summed, explicit zeros dropped, rows sorted,
    fp64 values."""
    A = ssp.csr_matrix(A, copy=True)
    if A.shape[0] != A.shape[1]:
        raise ValueError(f"A must be square, got {A.shape}")
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return ssp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)


def check_links(edge_index, num_nodes):
    """edge_index [2, L] (tensor or array, any integer type) -> int64 numpy [2, L]; ValueError on a bad shape or
    a node outside [0, num_nodes)."""
    ei = edge_index.detach().cpu().numpy() if isinstance(edge_index, torch.Tensor) else np.asarray(edge_index)
    if ei.size == 0:
        return np.zeros((2, 0), dtype=np.int64)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError(f"edge_index must be [2, L], got {tuple(ei.shape)}")
    if not np.issubdtype(ei.dtype, np.integer):
        raise ValueError(f"edge_index must hold integer node ids, got {ei.dtype}")
    ei = ei.astype(np.int64, copy=False)
    if ei.min() < 0 or ei.max() >= num_nodes:
        raise ValueError(f"edge_index holds a node outside [0, {num_nodes})")
    return ei


def check_block_width(block_width):
    bw = int(block_width)
    if bw and (bw < 64 or bw > 1024 or bw % 64):
        raise ValueError("block_width must be 0 or a multiple of 64 in [64, 1024]")
    return bw


def check_katz(beta, max_len, block_width=0):
    """(beta, max_len, block_width) as the kernels take them; ValueError outside the envelope (beta finite,
    1 <= max_len <= 64, block_width 0 or a multiple of 64 up to 1024)."""
    if isinstance(max_len, bool) or not isinstance(max_len, (int, np.integer)):
        raise ValueError(f"max_len must be an integer, got {max_len!r}")
    if not np.isfinite(float(beta)) or not 1 <= int(max_len) <= KATZ_MAX_LEN:
        raise ValueError(f"need a finite beta and 1 <= max_len <= {KATZ_MAX_LEN}, got {beta!r} and {max_len!r}")
    return float(beta), int(max_len), check_block_width(block_width)


class Heuristics:
    """A graph on the device with its CN / AA / PPR / RA / Jaccard / PA / Katz scorers.  Registered with its engine,
    which closes it."""

    def __init__(self, A, device=None):
        A = canonical_csr(A)
        n = A.shape[0]
        if n < 1 or n >= 1 << 31 or A.nnz >= 1 << 31:
            raise ValueError(f"need 1 <= N < 2^31 and nnz < 2^31, got N = {n}, nnz = {A.nnz}")
        from .engine import default_engine

        self.engine = default_engine(device)
        dev = self.engine.device
        self.num_nodes = n
        ip = torch.as_tensor(A.indptr.astype(np.int64)).to(dev)
        ix = torch.as_tensor(A.indices.astype(np.int32)).to(dev)
        vx = torch.as_tensor(A.data).to(dev)
        h = C.c_void_p()
        N.check(N.lib().s3grl_heuristics_create(self.engine._ctx, n, N.ptr(ip), N.ptr(ix), N.ptr(vx), int(A.nnz),
                                                C.byref(h)), "s3grl_heuristics_create")
        self._h = h
        self.engine._children.add(self)   # the engine closes it before its context goes

    def _links(self, links):
        ei = check_links(links, self.num_nodes)
        return torch.as_tensor(ei.astype(np.int32)).to(self.engine.device).contiguous()

    def _pairs(self, kind, links):
        self._alive()
        ei = self._links(links)
        L = ei.shape[1]
        out = torch.empty(L, dtype=torch.float32, device=self.engine.device)
        if L:
            N.check(N.lib().s3grl_heuristics_pairs(self._h, KIND[kind], N.ptr(ei), L, N.ptr(out)),
                    "s3grl_heuristics_pairs")
        return out

    def cn(self, links):
        """Common neighbours of every link of `links` [2, L]: fp32 [L] on the device."""
        return self._pairs("CN", links)

    def aa(self, links):
        """Adamic-Adar of every link of `links` [2, L]: fp32 [L] on the device."""
        return self._pairs("AA", links)

    def ppr(self, links, p=0.85, tol=1e-7, max_iter=100, return_iterations=False, block_width=0):
        """Personalised PageRank x_s[d] of every link (s, d) of `links` [2, L], in the given order: fp32 [L] on the
        device.  Each distinct source is solved once.  `return_iterations` also returns int32 [L]: the iterations
        the link's source ran.  `block_width` (sources per block, a multiple of 64 up to 1024; 0: the default)
        changes the speed only, never a result."""
        self._alive()
        if not 0.0 <= float(p) <= 1.0 or not float(tol) >= 0.0 or int(max_iter) < 1:
            raise ValueError("need 0 <= p <= 1, tol >= 0 and max_iter >= 1")
        bw = check_block_width(block_width)
        ei = check_links(links, self.num_nodes)
        dev = self.engine.device
        L = ei.shape[1]
        src, inv = np.unique(ei[0], return_inverse=True)
        out = torch.empty(L, dtype=torch.float32, device=dev)
        its = torch.zeros(len(src), dtype=torch.int32, device=dev)
        if L:
            s_d = torch.as_tensor(src.astype(np.int32)).to(dev)
            l_d = torch.as_tensor(ei.astype(np.int32)).to(dev).contiguous()
            N.check(N.lib().s3grl_heuristics_ppr(self._h, N.ptr(s_d), len(src), N.ptr(l_d), L, float(p), float(tol),
                                                 int(max_iter), bw, N.ptr(out), N.ptr(its)), "s3grl_heuristics_ppr")
        if return_iterations:
            return out, its[torch.as_tensor(inv.reshape(-1).astype(np.int64)).to(dev)]
        return out

    def ra(self, links):
        """Resource allocation of every link of `links` [2, L]: fp32 [L] on the device."""
        return self._pairs("RA", links)

    def jaccard(self, links):
        """Structural Jaccard coefficient of every link of `links` [2, L]: fp32 [L] on the device."""
        return self._pairs("JACCARD", links)

    def pa(self, links):
        """Preferential attachment r_s·r_d of every link of `links` [2, L]: fp32 [L] on the device."""
        return self._pairs("PA", links)

    def katz(self, links, beta=0.005, max_len=3, block_width=0):
        """Truncated Katz index Σ_{l=1..max_len} β^l·(A^l)[s, d] of every link (s, d) of `links` [2, L], in the
        given order: fp32 [L] on the device.  Each distinct source is solved once.  `block_width` as for `ppr`:
        it changes the speed only, never a result."""
        beta, max_len, bw = check_katz(beta, max_len, block_width)
        ei = check_links(links, self.num_nodes)
        self._alive()
        dev = self.engine.device
        L = ei.shape[1]
        out = torch.empty(L, dtype=torch.float32, device=dev)
        if L:
            src = np.unique(ei[0])
            s_d = torch.as_tensor(src.astype(np.int32)).to(dev)
            l_d = torch.as_tensor(ei.astype(np.int32)).to(dev).contiguous()
            N.check(N.lib().s3grl_heuristics_katz(self._h, N.ptr(s_d), len(src), N.ptr(l_d), L, beta, max_len, bw,
                                                  N.ptr(out)), "s3grl_heuristics_katz")
        return out

    def _alive(self):
        if getattr(self, "_h", None) is None:
            raise RuntimeError("Heuristics is closed")

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and self.engine._ctx:   # the object works on the context's stream
            N.lib().s3grl_heuristics_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _as_index_tensor(edge_index):
    return edge_index if isinstance(edge_index, torch.Tensor) else torch.as_tensor(np.asarray(edge_index))


def _pair_twin(kind, A, edge_index):
    ei = check_links(edge_index, A.shape[0])
    h = Heuristics(A)
    try:
        scores = h._pairs(kind, ei).cpu()
    finally:
        h.close()
    return scores, _as_index_tensor(edge_index)


def CN(A, edge_index, batch_size=100000):
    """Reference utils.CN: (fp32 CPU scores [L], edge_index).  `batch_size` is accepted and changes nothing."""
    return _pair_twin("CN", A, edge_index)


def AA(A, edge_index, batch_size=100000):
    """Reference utils.AA: (fp32 CPU scores [L], edge_index).  `batch_size` is accepted and changes nothing."""
    return _pair_twin("AA", A, edge_index)


def RA(A, edge_index, batch_size=100000):
    """Resource allocation with `CN`'s signature: (fp32 CPU scores [L], edge_index)."""
    return _pair_twin("RA", A, edge_index)


def Jaccard(A, edge_index, batch_size=100000):
    """Structural Jaccard coefficient with `CN`'s signature: (fp32 CPU scores [L], edge_index)."""
    return _pair_twin("JACCARD", A, edge_index)


def PA(A, edge_index, batch_size=100000):
    """Preferential attachment with `CN`'s signature: (fp32 CPU scores [L], edge_index)."""
    return _pair_twin("PA", A, edge_index)


def Katz(A, edge_index, beta=0.005, max_len=3):
    """Truncated Katz index: (fp32 CPU scores [L], edge_index), in the given order (unlike `PPR`, no reorder)."""
    check_katz(beta, max_len)
    ei = check_links(edge_index, A.shape[0])
    h = Heuristics(A)
    try:
        scores = h.katz(ei, beta, max_len).cpu()
    finally:
        h.close()
    return scores, _as_index_tensor(edge_index)


def PPR(A, edge_index):
    """Reference utils.PPR: (fp32 CPU scores [L], edge_index reordered by source).  The reorder is a STABLE sort by
    source (the reference's torch.sort is not stable, so its order among links of one source is unspecified)."""
    ei = check_links(edge_index, A.shape[0])
    order = np.argsort(ei[0], kind="stable")
    ei = ei[:, order]
    h = Heuristics(A)
    try:
        scores = h.ppr(ei).cpu()
    finally:
        h.close()
    return scores, torch.as_tensor(ei)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _curve(y_true, y_score):
    """sklearn's _binary_clf_curve: true and false positives at each distinct threshold, highest first."""
    y = _np(y_true).reshape(-1) == 1
    s = _np(y_score).reshape(-1).astype(np.float64)
    order = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[order], y[order]
    last = np.r_[np.where(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y)[last].astype(np.float64)
    return tps, 1.0 + last - tps


def roc_auc(y_true, y_score):
    """sklearn.metrics.roc_auc_score (binary): the trapezoid under the ROC curve, ties as one step."""
    tps, fps = _curve(y_true, y_score)
    if tps[-1] == 0 or fps[-1] == 0:
        raise ValueError("AUC needs both classes in y_true")
    tpr, fpr = np.r_[0.0, tps / tps[-1]], np.r_[0.0, fps / fps[-1]]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def average_precision(y_true, y_score):
    """sklearn.metrics.average_precision_score: Σ (R_i − R_{i−1})·P_i over the distinct thresholds."""
    tps, fps = _curve(y_true, y_score)
    if tps[-1] == 0:
        raise ValueError("AP needs a positive in y_true")
    precision, recall = tps / (tps + fps), tps / tps[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def evaluate_auc(val_pred, val_true, test_pred, test_true):
    """Reference utils.evaluate_auc: {'AUC': (val, test), 'AP': (val, test)}, as sklearn computes them."""
    return {"AUC": (roc_auc(val_true, val_pred), roc_auc(test_true, test_pred)),
            "AP": (average_precision(val_true, val_pred), average_precision(test_true, test_pred))}


def run_heuristic(split, name, device=None, **kw):
    """One Table 2 heuristic row from a `workloads.Split`: the four val/test lists scored on the train graph
    `split.A` with one `Heuristics`, then `evaluate_auc`.  PPR and KATZ solve every distinct source of the four
    lists once, and take `kw` (`ppr`'s or `katz`'s keyword arguments).
    Returns {'AUC': (val, test), 'AP': (val, test)}."""
    name = name.upper()
    if name not in NAMES:
        raise ValueError(f"unknown heuristic {name!r}: one of {NAMES}")
    if name == "KATZ":
        check_katz(kw.get("beta", 0.005), kw.get("max_len", 3), kw.get("block_width", 0))
    lists = [split.links["valid"][0], split.links["valid"][1], split.links["test"][0], split.links["test"][1]]
    lists = [check_links(x, split.num_nodes) for x in lists]
    h = Heuristics(split.A, device)
    try:
        if name == "PPR":
            scores = h.ppr(np.concatenate(lists, axis=1), **kw).cpu().numpy()
        elif name == "KATZ":
            scores = h.katz(np.concatenate(lists, axis=1), **kw).cpu().numpy()
        else:
            scores = h._pairs(name, np.concatenate(lists, axis=1)).cpu().numpy()
    finally:
        h.close()
    parts = np.split(scores, np.cumsum([x.shape[1] for x in lists])[:-1])
    val_pred, test_pred = np.concatenate(parts[:2]), np.concatenate(parts[2:])
    val_true = np.r_[np.ones(lists[0].shape[1]), np.zeros(lists[1].shape[1])]
    test_true = np.r_[np.ones(lists[2].shape[1]), np.zeros(lists[3].shape[1])]
    return evaluate_auc(val_pred, val_true, test_pred, test_true)
