"""Link-ranking metrics on the device: the four `--eval_metric` values of the reference (sgrl_link_pred.py:704-770:
`auc` = sklearn's roc_auc_score and average_precision_score, `hits` = OGB's Hits@20/50/100, `mrr` = OGB's MRR, `rocauc` =
OGB's ROC-AUC), as HIP kernels behind the C ABI (s3grl_metrics_*, csrc/s3grl_metrics.hip).

    m = LinkMetrics()
    r = m.ranked(scores, labels, ks=(20, 50, 100))   # {'AUC', 'AP', 'hits': {K: fraction}, 'num_pos', 'num_neg', 'thresholds'}
    h = m.hits(pos, neg)                             # {20: .., 50: .., 100: ..}
    q = m.mrr(pos, neg)                              # {'MRR', 'mrr_list', 'hits@1', 'hits@3', 'hits@10'}
    evaluate_auc(val_pred, val_true, test_pred, test_true)       # the reference's functions, same result shapes

Definitions.  Scores are taken as fp32.  Sorted by descending score, equal scores (−0.0 equals +0.0; ±inf are values) form
one threshold; with tp, fp the positives and negatives at or above a threshold, P and N their totals:

- AUC is the trapezoid under (fp / N, tp / P), summed as the exact integer Σ fp_g (2 tp_b + tp_g) over the thresholds
  (tp_b the positives above the threshold's group, tp_g / fp_g those in it) and divided once by 2 P N.
- AP = Σ (tp_g / P) · tp / (tp + fp) over the thresholds, in fp64 in a fixed order.
- Hits@K (OGB): 1.0 with fewer than K negatives, else the share of positives strictly above the K-th largest negative.
- MRR (OGB, tie-aware): per positive and its M negatives rank = (#{neg > pos} + #{neg >= pos}) / 2 + 1, mrr = 1 / rank in
  fp32; 'MRR' is the fp64 mean of the list; hits@J the share of rank <= J.

Two calls on one input give the same bits.  GPU only; there is no CPU fallback.  Device tensors are read in place; CPU
tensors and numpy arrays are uploaded (and, being on the host anyway, checked there first).
"""
from __future__ import annotations

import ctypes as ct

import numpy as np
import torch

from . import _native as N

MRR_HITS = (1, 3, 10)


def layout(num_neg=1):
    """The work split of the kernels, without a GPU: dict(block_items: sorted scores per workgroup of the scan passes;
    rows_per_wave, lanes_per_row, rows_per_block: of the MRR kernel for rows of num_neg negatives; vector_width: floats
    per load; max_ks: the most K values of one `ranked` call)."""
    num_neg = int(num_neg)
    if not 1 <= num_neg < 1 << 31:
        raise ValueError(f"num_neg must be in [1, 2^31), got {num_neg}")
    out = (ct.c_int32 * 6)()
    N.check(N.lib().s3grl_metrics_layout(num_neg, out), "s3grl_metrics_layout")
    return {"block_items": out[0], "rows_per_wave": out[1], "lanes_per_row": out[2], "vector_width": out[3],
            "max_ks": out[4], "rows_per_block": out[5]}


# -- argument checks that need no device ------------------------------------------------------------------------------
def _on_host(x):
    return not (isinstance(x, torch.Tensor) and x.device.type != "cpu")


def _flat(x, what):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if t.dim() == 0:
        raise ValueError(f"{what} must be an array, got a scalar")
    return t.detach().reshape(-1)


def _check_ks(ks):
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError(f"every K must be at least 1, got {ks}")
    if len(set(ks)) != len(ks):
        raise ValueError(f"K values must be distinct, got {ks}")
    return ks


def _no_nan(t, what):
    if _on_host(t) and t.is_floating_point() and bool(torch.isnan(t).any()):
        raise ValueError(f"{what} contains NaN")


def _ranked_args(scores, labels, ks):
    """(scores [n], labels [n], ks) checked as far as the host can: shapes always, values when the data is on the
    host."""
    s, y, ks = _flat(scores, "scores"), _flat(labels, "labels"), _check_ks(ks)
    if s.numel() != y.numel():
        raise ValueError(f"need one label per score, got {y.numel()} labels for {s.numel()} scores")
    if s.numel() >= 1 << 31:
        raise ValueError(f"at most 2^31 - 1 scores, got {s.numel()}")
    _no_nan(s, "scores")
    if _on_host(y) and y.numel():
        ok = (y == 1) | (y == 0)
        if not bool(ok.all()):
            raise ValueError("labels must be 0 or 1")
        _classes(int((y == 1).sum()), y.numel() - int((y == 1).sum()))
    elif not y.numel():
        _classes(0, 0)
    return s, y, ks


def _classes(num_pos, num_neg, need_neg=True):
    if num_pos == 0:
        raise ValueError("AP, Hits@K and MRR need a positive in y_true")
    if need_neg and num_neg == 0:
        raise ValueError("AUC needs both classes in y_true")


def _pos_neg_args(pos, neg):
    p, q = _flat(pos, "pos"), _flat(neg, "neg")
    if p.numel() == 0:
        _classes(0, q.numel())
    if p.numel() + q.numel() >= 1 << 31:
        raise ValueError(f"at most 2^31 - 1 scores, got {p.numel() + q.numel()}")
    _no_nan(p, "pos")
    _no_nan(q, "neg")
    return p, q


def _mrr_args(pos, neg):
    p = _flat(pos, "pos")
    q = neg if isinstance(neg, torch.Tensor) else torch.as_tensor(np.asarray(neg))
    q = q.detach()
    if p.numel() == 0:
        _classes(0, q.numel())
    if q.dim() not in (1, 2) or (q.dim() == 2 and q.shape[0] != p.numel()):
        raise ValueError(f"neg must be [{p.numel()}, M] or flat [{p.numel()} * M], got {tuple(q.shape)}")
    if q.numel() == 0 or q.numel() % p.numel():
        raise ValueError(f"neg must hold M >= 1 scores per positive: {q.numel()} scores for {p.numel()} positives")
    if p.numel() >= 1 << 31 or q.numel() // p.numel() >= 1 << 31:
        raise ValueError("at most 2^31 - 1 positives and negatives per positive")
    _no_nan(p, "pos")
    _no_nan(q, "neg")
    return p, q.reshape(p.numel(), -1)


class LinkMetrics:
    """AUC, AP, Hits@K and MRR of scores on the device.  Owns a workspace that grows with the largest call; registered
    with its engine, which closes it."""

    def __init__(self, device=None):
        if device is not None and torch.device(device).type == "cpu":
            raise RuntimeError("the link metrics need a HIP device (MI355X); there is no CPU fallback")
        from .engine import default_engine

        self.engine = default_engine(device)
        h = ct.c_void_p()
        N.check(N.lib().s3grl_metrics_create(self.engine._ctx, ct.byref(h)), "s3grl_metrics_create")
        self._h = h
        self.engine._children.add(self)   # the engine closes it before its context goes

    # -- the one sort ------------------------------------------------------------------------------------------
    def _scores(self, t):
        return t.to(device=self.engine.device, dtype=torch.float32).contiguous()

    def _labels(self, y):
        """uint8 on the device: 1, 0, and 2 for anything else (the key kernel counts those)."""
        y = y.to(self.engine.device)
        if y.dtype == torch.bool:
            return y.to(torch.uint8).contiguous()
        two = torch.full((), 2, dtype=torch.uint8, device=y.device)
        return torch.where(y == 1, 1, torch.where(y == 0, 0, two)).to(torch.uint8).contiguous()

    def _sort(self, s, y8, n_pos, ks):
        """One s3grl_metrics_ranked call -> (P, N, thresholds, AUC numerator, AP, {K: count or -1}); ValueError for NaN
        scores and bad labels."""
        self._alive()
        if len(ks) > layout()["max_ks"]:
            raise ValueError(f"at most {layout()['max_ks']} K values per call, got {len(ks)}")
        counts, ap = (ct.c_int64 * 6)(), ct.c_double()
        kbuf, hbuf = (ct.c_int64 * max(len(ks), 1))(*ks), (ct.c_int64 * max(len(ks), 1))()
        N.check(N.lib().s3grl_metrics_ranked(self._h, N.ptr(s), N.ptr(y8), s.numel(), int(n_pos), kbuf, len(ks), counts,
                                             ct.byref(ap), hbuf), "s3grl_metrics_ranked")
        if counts[3]:
            raise ValueError(f"scores contain NaN ({counts[3]} of {s.numel()})")
        if counts[4]:
            raise ValueError("labels must be 0 or 1")
        return counts[0], counts[1], counts[2], counts[5], ap.value, {k: hbuf[i] for i, k in enumerate(ks)}

    @staticmethod
    def _fractions(hits, num_pos, num_neg):
        return {k: 1.0 if num_neg < k else c / num_pos for k, c in hits.items()}

    def ranked(self, scores, labels=None, ks=(), *, n_pos=None):
        """AUC, AP and Hits@K of scores [n] from one sort: {'AUC', 'AP', 'hits': {K: fraction}, 'num_pos', 'num_neg',
        'thresholds'}.  Either labels [n] (int, bool, uint8 or float holding 0 / 1) or n_pos: the first n_pos scores are
        the positives, the rest the negatives.  ValueError without both classes."""
        if (labels is None) == (n_pos is None):
            raise ValueError("give either labels or n_pos")
        if labels is None:
            s, n_pos = _flat(scores, "scores"), int(n_pos)
            if not 0 <= n_pos <= s.numel():
                raise ValueError(f"n_pos must be in [0, {s.numel()}], got {n_pos}")
            return self._ranked_split(s[:n_pos], s[n_pos:], ks, whole=s)
        s, y, ks = _ranked_args(scores, labels, ks)
        P, Nn, thr, num, ap, hits = self._sort(self._scores(s), self._labels(y), 0, ks)
        _classes(P, Nn)
        return {"AUC": num / (2 * P * Nn), "AP": ap, "hits": self._fractions(hits, P, Nn), "num_pos": P, "num_neg": Nn,
                "thresholds": thr}

    def _ranked_split(self, pos, neg, ks=(), whole=None):
        """`ranked` of positives and negatives given apart, or as the two ends of `whole` (the n_pos form, which needs
        both classes); given apart N = 0 is allowed and 'AUC' is then None."""
        p, q = _pos_neg_args(pos, neg)
        ks = _check_ks(ks)
        if whole is not None:
            _classes(p.numel(), q.numel())
        s = self._scores(whole) if whole is not None else torch.cat([self._scores(p), self._scores(q)])
        P, Nn, thr, num, ap, hits = self._sort(s, None, p.numel(), ks)
        return {"AUC": num / (2 * P * Nn) if Nn else None, "AP": ap, "hits": self._fractions(hits, P, Nn), "num_pos": P,
                "num_neg": Nn, "thresholds": thr}

    def hits(self, pos, neg, ks=(20, 50, 100)):
        """OGB's Hits@K: {K: 1.0 when len(neg) < K, else #{pos > K-th largest neg} / len(pos)}."""
        return self._ranked_split(pos, neg, ks)["hits"]

    def rocauc(self, pos, neg):
        """OGB's rocauc: sklearn's roc_auc_score of the positives against the negatives."""
        r = self._ranked_split(pos, neg)
        _classes(r["num_pos"], r["num_neg"])
        return r["AUC"]

    def mrr(self, pos, neg):
        """OGB's MRR of pos [P] against neg [P, M] (or flat [P * M], rows in order): {'MRR': the mean, 'mrr_list': fp32
        [P] on the device, 'hits@1', 'hits@3', 'hits@10'}."""
        self._alive()
        p, q = _mrr_args(pos, neg)
        p, q = self._scores(p), self._scores(q)
        P, M = q.shape
        out = torch.empty(P, dtype=torch.float32, device=self.engine.device)
        total, counts = ct.c_double(), (ct.c_int64 * 4)()
        N.check(N.lib().s3grl_metrics_mrr(self._h, N.ptr(p), N.ptr(q), P, M, N.ptr(out), ct.byref(total), counts),
                "s3grl_metrics_mrr")
        if counts[3]:
            raise ValueError(f"scores contain NaN ({counts[3]} of {P + P * M})")
        res = {"MRR": total.value / P, "mrr_list": out}
        res.update({f"hits@{j}": counts[i] / P for i, j in enumerate(MRR_HITS)})
        return res

    def _alive(self):
        if getattr(self, "_h", None) is None:
            raise RuntimeError("LinkMetrics is closed")

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and self.engine._ctx:   # it works on the context's stream
            N.lib().s3grl_metrics_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _shared(device=None):
    """One LinkMetrics per engine for the module-level functions, closed with the engine."""
    if device is not None and torch.device(device).type == "cpu":
        raise RuntimeError("the link metrics need a HIP device (MI355X); there is no CPU fallback")
    from .engine import default_engine

    eng = default_engine(device)
    m = getattr(eng, "_link_metrics", None)
    if m is None or m._h is None:
        m = eng._link_metrics = LinkMetrics(eng.device)
    return m


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.device.type != "cpu":
            return x.device
    return None


# -- the reference's functions (sgrl_link_pred.py:704-770) ----------------------------------------------------------------
def evaluate_auc(val_pred, val_true, test_pred, test_true):
    """{'AUC': (valid, test), 'AP': (valid, test)}: sklearn's roc_auc_score and average_precision_score."""
    args = [_ranked_args(val_pred, val_true, ()), _ranked_args(test_pred, test_true, ())]
    m = _shared(_device_of(val_pred, val_true, test_pred, test_true))
    v, t = (m.ranked(s, y) for s, y, _ in args)
    return {"AUC": (v["AUC"], t["AUC"]), "AP": (v["AP"], t["AP"])}


def evaluate_hits(pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred, evaluator=None):
    """{'Hits@20': (valid, test), 'Hits@50': …, 'Hits@100': …} by OGB's rule.  `evaluator` is accepted and ignored."""
    args = [_pos_neg_args(pos_val_pred, neg_val_pred), _pos_neg_args(pos_test_pred, neg_test_pred)]
    m = _shared(_device_of(pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred))
    v, t = (m.hits(p, q) for p, q in args)
    return {f"Hits@{k}": (v[k], t[k]) for k in (20, 50, 100)}


def evaluate_mrr(pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred, evaluator=None):
    """{'MRR': (valid, test)}: the mean of OGB's mrr_list, the negatives viewed as [len(pos), -1].  `evaluator` is
    accepted and ignored."""
    args = [_mrr_args(pos_val_pred, neg_val_pred), _mrr_args(pos_test_pred, neg_test_pred)]
    m = _shared(_device_of(pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred))
    v, t = (m.mrr(p, q)["MRR"] for p, q in args)
    return {"MRR": (v, t)}


def evaluate_ogb_rocauc(pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred, evaluator=None):
    """{'rocauc': (valid, test)}.  `evaluator` is accepted and ignored."""
    args = [_pos_neg_args(pos_val_pred, neg_val_pred), _pos_neg_args(pos_test_pred, neg_test_pred)]
    for p, q in args:
        _classes(p.numel(), q.numel())
    m = _shared(_device_of(pos_val_pred, neg_val_pred, pos_test_pred, neg_test_pred))
    v, t = (m.rocauc(p, q) for p, q in args)
    return {"rocauc": (v, t)}
