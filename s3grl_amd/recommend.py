"""Top-K link recommendation: for these nodes, which new links are most likely?

    seg_ptr, cand = candidates(graph, sources, hops=2)          # every node at distance 2..hops of each source
    top = recommend(graph, sources, SignScorer(eng, graph, feat, trainer, num_hops=1, sign_k=2), k=10)
    top.nodes, top.scores, top.count                            # int32 [S, k] (-1), fp32 [S, k] (-inf), int32 [S]

Two HIP kernels behind the C ABI (csrc/s3grl_recommend.hip) frame code that exists: `candidates` enumerates the
pairs (s3grl_candidates_count / _fill), a scorer — the engine's precompute and a trained SIGNNet, or a heuristic —
gives one fp32 score per pair, and `segment_topk` (s3grl_segment_topk) keeps the k best per source.

- Segment i of `candidates` holds, in ascending node id, every v with 2 <= dist(sources[i], v) <= hops on the graph
  as given: never the source itself, never a neighbour, and no v whose pair with the source is in `exclude` (either
  orientation).  A source listed twice gets two segments.
- `segment_topk` orders a segment by score descending, then position ascending (so ties go to the lower node id);
  -0.0 counts as +0.0 and a NaN ranks below -inf: `numpy.lexsort((position, -score))` with the NaNs moved last.
- `recommend` counts once, cuts the sources into consecutive chunks whose candidate totals stay within `chunk_pairs`
  (a single source above the cap is a chunk of its own) and per chunk fills, scores and ranks into its rows of the
  output; no chunk's pairs, rows or scores outlive it.

GPU only; there is no CPU fallback.  Bad arguments raise ValueError naming the argument before any GPU work.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _native as N


class TopK(NamedTuple):
    nodes: torch.Tensor    # int32 [S, k], padded with -1
    scores: torch.Tensor   # fp32 [S, k], padded with -inf
    count: torch.Tensor    # int32 [S] = min(k, candidates of the source)


# ---- argument checks (host; no GPU needed) ---------------------------------------------------------------------
def _check_hops(hops):
    if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or hops < 2:
        raise ValueError(f"hops must be an integer >= 2 (distance 1 is the graph itself), got {hops!r}")
    if hops > N.CANDIDATES_MAX_HOPS:
        raise ValueError(f"hops must be <= {N.CANDIDATES_MAX_HOPS}, got {hops}")
    return int(hops)


def _check_k(k):
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"k must be an integer >= 1, got {k!r}")
    return int(k)


def _check_sources(sources, num_nodes):
    """-> a 1-d integer tensor (where it was), every id inside [0, num_nodes)."""
    if isinstance(sources, (list, tuple)) and len(sources) == 0:
        sources = np.zeros(0, dtype=np.int64)          # an empty sequence has no dtype of its own (numpy: float64)
    s = sources if isinstance(sources, torch.Tensor) else torch.as_tensor(np.asarray(sources))
    if s.dtype.is_floating_point or s.dtype.is_complex or s.dtype == torch.bool:
        raise ValueError(f"sources must hold integer node ids, got {s.dtype}")
    if s.dim() != 1:
        raise ValueError(f"sources must be [S], got {tuple(s.shape)}")
    if s.numel() and (int(s.min()) < 0 or int(s.max()) >= num_nodes):
        raise ValueError(f"sources holds a node outside [0, {num_nodes})")
    return s


def _check_exclude(exclude, num_nodes):
    """-> None, or an int64 tensor [2, E] (where it was) of ids inside [0, num_nodes)."""
    if exclude is None:
        return None
    e = exclude if isinstance(exclude, torch.Tensor) else torch.as_tensor(np.asarray(exclude))
    if e.dim() != 2 or e.shape[0] != 2:
        raise ValueError(f"exclude must be [2, E], got {tuple(e.shape)}")
    if e.dtype.is_floating_point or e.dtype.is_complex or e.dtype == torch.bool:
        raise ValueError(f"exclude must hold integer node ids, got {e.dtype}")
    if e.numel() and (int(e.min()) < 0 or int(e.max()) >= num_nodes):
        raise ValueError(f"exclude holds a node outside [0, {num_nodes})")
    return e.to(torch.int64)


def _check_scores(scores, num_pairs):
    if not isinstance(scores, torch.Tensor):
        raise ValueError(f"scores must be a tensor, got {type(scores).__name__}")
    if scores.dtype != torch.float32:
        raise ValueError(f"scores must be fp32, got {scores.dtype}")
    if scores.dim() != 1 or scores.numel() != num_pairs:
        raise ValueError(f"scores must be [{num_pairs}], one per candidate, got {tuple(scores.shape)}")
    return scores


def _check_segments(seg_ptr, cand):
    if not isinstance(seg_ptr, torch.Tensor) or seg_ptr.dtype != torch.int64 or seg_ptr.dim() != 1 or \
            seg_ptr.numel() < 1:
        raise ValueError("seg_ptr must be an int64 tensor [S + 1]")
    if not isinstance(cand, torch.Tensor) or cand.dtype != torch.int32 or cand.dim() != 1:
        raise ValueError("cand must be an int32 tensor [P]")


def _chunks(seg_ptr, chunk_pairs):
    """Consecutive source ranges [a, b) whose candidate totals stay within chunk_pairs; a single source above the
    cap is a range of its own.  seg_ptr: host int64 [S + 1]."""
    S, a, out = len(seg_ptr) - 1, 0, []
    while a < S:
        b = int(np.searchsorted(seg_ptr, seg_ptr[a] + chunk_pairs, side="right")) - 1
        b = min(max(b, a + 1), S)
        out.append((a, b))
        a = b
    return out


def layout(num_nodes, hops=2):
    """How `candidates` lays a source's walk out on a graph of num_nodes nodes, without a GPU: dict(bitmap "lds" or
    "hbm", bitmap_words (of one of the two bitmaps), threads per workgroup, lds_bytes per workgroup, workspace_bytes
    per resident workgroup, resident_workgroups (0: one workgroup per source), lds_nodes: the bound of the LDS
    flavour)."""
    if isinstance(num_nodes, bool) or not isinstance(num_nodes, (int, np.integer)) or not 1 <= num_nodes < 1 << 31:
        raise ValueError(f"num_nodes must be an integer in [1, 2^31), got {num_nodes!r}")
    hops = _check_hops(hops)
    out = (C.c_int64 * 8)()
    N.check(N.lib().s3grl_candidates_layout(int(num_nodes), hops, out), "s3grl_candidates_layout")
    return {"bitmap": "hbm" if out[0] else "lds", "bitmap_words": int(out[1]), "threads": int(out[2]),
            "lds_bytes": int(out[3]), "workspace_bytes": int(out[4]), "resident_workgroups": int(out[5]),
            "lds_nodes": int(out[6])}


# ---- the two kernels -------------------------------------------------------------------------------------------
def _exclude_keys(exclude, num_nodes, device):
    """Sorted unique keys min * N + max as int64 on the device (below 2^62: the same order as the uint64 the ABI reads)."""
    if exclude is None or exclude.numel() == 0:
        return None
    e = exclude.to(device)
    keys = torch.minimum(e[0], e[1]) * num_nodes + torch.maximum(e[0], e[1])
    return torch.unique(keys, sorted=True).contiguous()


def _prepare(graph, sources, hops, exclude):
    hops = _check_hops(hops)
    src = _check_sources(sources, graph.num_nodes)
    exclude = _check_exclude(exclude, graph.num_nodes)
    if graph.directed:
        raise NotImplementedError("candidates: directed graphs are not implemented")
    dev = graph.engine.device
    return src.to(device=dev, dtype=torch.int32).contiguous(), hops, _exclude_keys(exclude, graph.num_nodes, dev)


def _count(graph, src, hops, keys):
    eng = graph.engine
    seg_ptr = torch.empty(src.numel() + 1, dtype=torch.int64, device=eng.device)
    total = C.c_int64()
    N.check(N.lib().s3grl_candidates_count(eng._ctx, graph._h, N.ptr(src), src.numel(), hops, N.ptr(keys),
                                           0 if keys is None else keys.numel(), N.ptr(seg_ptr), C.byref(total)),
            "s3grl_candidates_count")
    return seg_ptr, int(total.value)


def _fill(graph, src, hops, keys, seg_ptr, total):
    eng = graph.engine
    cand = torch.empty(total, dtype=torch.int32, device=eng.device)
    N.check(N.lib().s3grl_candidates_fill(eng._ctx, graph._h, N.ptr(src), src.numel(), hops, N.ptr(keys),
                                          0 if keys is None else keys.numel(), N.ptr(seg_ptr), N.ptr(cand)),
            "s3grl_candidates_fill")
    return cand


def candidates(graph, sources, hops=2, exclude=None):
    """(seg_ptr int64 [S + 1], cand int32 [seg_ptr[S]]) on the device: per source, in ascending node id, every node at
    distance 2..hops.  `exclude`: int64 [2, E] pairs never to propose, any orientation, duplicates allowed."""
    src, hops, keys = _prepare(graph, sources, hops, exclude)
    seg_ptr, total = _count(graph, src, hops, keys)
    return seg_ptr, _fill(graph, src, hops, keys, seg_ptr, total)


def _topk_into(eng, scores, seg_ptr, cand, k, nodes, top_scores, count):
    S = seg_ptr.numel() - 1
    N.check(N.lib().s3grl_segment_topk(eng._ctx, N.ptr(scores), N.ptr(seg_ptr), N.ptr(cand), cand.numel(), S, k,
                                       N.ptr(nodes), N.ptr(top_scores), N.ptr(count)), "s3grl_segment_topk")


def segment_topk(scores, seg_ptr, cand, k, engine=None):
    """The k best candidates of every segment: TopK(nodes, scores, count).  scores fp32 [P], cand int32 [P] and seg_ptr
    int64 [S + 1] (rising from 0 to at most P) on the device; 1 <= k <= 1024 (beyond: NotImplementedError)."""
    k = _check_k(k)
    _check_segments(seg_ptr, cand)
    scores = _check_scores(scores, cand.numel())
    if engine is None:
        from .engine import default_engine

        engine = default_engine(scores.device if scores.is_cuda else None)
    dev = engine.device
    scores, seg_ptr, cand = (t.to(dev).contiguous() for t in (scores, seg_ptr, cand))
    S = seg_ptr.numel() - 1
    top = TopK(torch.empty((S, k), dtype=torch.int32, device=dev), torch.empty((S, k), dtype=torch.float32, device=dev),
               torch.empty(S, dtype=torch.int32, device=dev))
    _topk_into(engine, scores, seg_ptr, cand, k, *top)
    return top


# ---- scorers: pairs int64 [2, P] on the device -> fp32 [P] on the device ----------------------------------------
class SignScorer:
    """The engine's precompute of the pairs, scored by a trained `SIGNNetTrainer` (eval mode)."""

    def __init__(self, engine, graph, features, trainer, mode="pos", num_hops=1, sign_k=3, strategy="intersection"):
        self.engine, self.graph, self.features, self.trainer = engine, graph, features, trainer
        self.kw = dict(mode=mode, num_hops=num_hops, sign_k=sign_k, strategy=strategy)

    def __call__(self, pairs):
        res = self.engine.precompute(self.graph, self.features, pairs.t().contiguous(), **self.kw)
        return self.trainer.score(res.rows, res.row_ptr)


class HeuristicScorer:
    """One index of a `Heuristics` object: "CN", "AA", "RA", "JACCARD", "PA", or "KATZ" (with `beta` and `max_len`
    in `kw`, solved once per source of a chunk)."""

    KINDS = ("CN", "AA", "RA", "JACCARD", "PA", "KATZ")

    def __init__(self, heuristics, kind, **kw):
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {self.KINDS}, got {kind!r}")
        if kind == "KATZ":
            from .heuristics import check_katz

            check_katz(kw.get("beta", 0.005), kw.get("max_len", 3), kw.get("block_width", 0))
            if set(kw) - {"beta", "max_len", "block_width"}:
                raise ValueError(f"kind 'KATZ' takes beta, max_len and block_width, got {sorted(kw)}")
        elif kw:
            raise ValueError(f"kind {kind!r} takes no keyword arguments, got {sorted(kw)}")
        self.heuristics, self.kind, self.kw = heuristics, kind, kw

    def __call__(self, pairs):
        if self.kind == "KATZ":
            return self.heuristics.katz(pairs, **self.kw)
        return self.heuristics._pairs(self.kind, pairs)


def recommend(graph, sources, scorer, k=10, hops=2, exclude=None, chunk_pairs=1 << 20):
    """TopK of every source among its candidates (see `candidates`), scored by `scorer`."""
    k = _check_k(k)
    if isinstance(chunk_pairs, bool) or not isinstance(chunk_pairs, (int, np.integer)) or chunk_pairs < 1:
        raise ValueError(f"chunk_pairs must be an integer >= 1, got {chunk_pairs!r}")
    src, hops, keys = _prepare(graph, sources, hops, exclude)
    if k > N.TOPK_MAX_K:
        raise NotImplementedError(f"recommend: k <= {N.TOPK_MAX_K}")
    eng, dev, S = graph.engine, graph.engine.device, src.numel()
    seg_ptr, _ = _count(graph, src, hops, keys)
    top = TopK(torch.empty((S, k), dtype=torch.int32, device=dev), torch.empty((S, k), dtype=torch.float32, device=dev),
               torch.empty(S, dtype=torch.int32, device=dev))
    ptr_h = seg_ptr.cpu().numpy()
    for a, b in _chunks(ptr_h, int(chunk_pairs)):
        P = int(ptr_h[b] - ptr_h[a])
        rel = (seg_ptr[a:b + 1] - seg_ptr[a]).contiguous()
        cand = _fill(graph, src[a:b], hops, keys, rel, P)
        if P:
            pairs = torch.stack([torch.repeat_interleave(src[a:b].long(), rel.diff(), output_size=P), cand.long()])
            scores = _check_scores(scorer(pairs), P).to(dev).contiguous()
            del pairs
        else:
            scores = torch.empty(0, dtype=torch.float32, device=dev)
        _topk_into(eng, scores, rel, cand, k, top.nodes[a:b], top.scores[a:b], top.count[a:b])
    return top


def recall_at_k(top, sources, targets):
    """The fraction of the held-out pairs (u, v) of `targets` [2, M], u among `sources`, whose v is in u's top-K: the
    full-ranking counterpart of Hits@K.  `sources` is the list `top` was computed for (a node listed twice: its first
    row).  NaN when no pair has its u among the sources.  Computed on the host."""
    nodes = top.nodes.detach().cpu().numpy()
    src = np.asarray(sources.detach().cpu() if isinstance(sources, torch.Tensor) else sources).reshape(-1)
    tg = np.asarray(targets.detach().cpu() if isinstance(targets, torch.Tensor) else targets)
    if tg.ndim != 2 or tg.shape[0] != 2:
        raise ValueError(f"targets must be [2, M], got {tuple(tg.shape)}")
    if len(src) != nodes.shape[0]:
        raise ValueError(f"sources must be [{nodes.shape[0]}], the list top was computed for, got {len(src)}")
    row = {}
    for i, u in enumerate(src.tolist()):
        row.setdefault(u, i)
    seen = hit = 0
    for u, v in tg.T.tolist():
        i = row.get(u)
        if i is None:
            continue
        seen += 1
        hit += int(v in nodes[i])
    return hit / seen if seen else float("nan")
