"""Plain numpy restatement of what s3grl_amd.metrics computes, for the host and the GPU tests.

Scores are compared as fp32 values (the kernels take fp32): equal values are one threshold, −0.0 equals +0.0, ±inf are
ordinary values.  AUC and AP are sklearn's (`_binary_clf_curve`), Hits@K is OGB's rule, MRR is the tie-aware form of OGB's
evaluator."""
import numpy as np


def _f32(x):
    return np.asarray(x, dtype=np.float32).reshape(-1)


def curve(y_true, y_score):
    """(tps, fps, thresholds) at each distinct threshold, highest first, as exact integers."""
    y = np.asarray(y_true).reshape(-1) == 1
    s = _f32(y_score).astype(np.float64)
    order = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[order], y[order]
    last = np.r_[np.where(s[1:] != s[:-1])[0], y.size - 1]     # not np.diff: inf − inf is NaN, and inf ties inf
    tps = np.cumsum(y.astype(np.int64))[last]
    return tps, 1 + last - tps, last.size


def roc_auc(y_true, y_score):
    """sklearn.metrics.roc_auc_score, by the trapezoid (`heuristics.roc_auc`, which this equals on finite scores)."""
    tps, fps, _ = curve(y_true, y_score)
    if tps[-1] == 0 or fps[-1] == 0:
        raise ValueError("AUC needs both classes in y_true")
    tpr, fpr = np.r_[0.0, tps / tps[-1]], np.r_[0.0, fps / fps[-1]]
    return float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))


def average_precision(y_true, y_score):
    """sklearn.metrics.average_precision_score (`heuristics.average_precision` on finite scores)."""
    tps, fps, _ = curve(y_true, y_score)
    if tps[-1] == 0:
        raise ValueError("AP needs a positive in y_true")
    precision, recall = tps / (tps + fps), tps / tps[-1]
    return float(np.sum(np.diff(np.r_[0.0, recall]) * precision))


def auc_numerator(y_true, y_score):
    """(Σ fp_g (2 tp_b + tp_g), P, N) in Python integers: the sum is 2·P·N·AUC exactly."""
    tps, fps, _ = curve(y_true, y_score)
    tps, fps = [0] + [int(v) for v in tps], [0] + [int(v) for v in fps]
    num = sum((fps[i] - fps[i - 1]) * (tps[i - 1] + tps[i]) for i in range(1, len(tps)))
    return num, tps[-1], fps[-1]


def roc_auc_exact(y_true, y_score):
    num, P, Nn = auc_numerator(y_true, y_score)
    if P == 0 or Nn == 0:
        raise ValueError("AUC needs both classes in y_true")
    return num / (2 * P * Nn)


def thresholds(y_score):
    return int(np.unique(_f32(y_score).astype(np.float64)).size)   # −0.0 == +0.0; inf == inf


def hits_count(pos, neg, K):
    """The positives strictly above the K-th largest negative, or None with fewer than K negatives."""
    pos, neg = _f32(pos), _f32(neg)
    if neg.size < K:
        return None
    kth = np.sort(neg)[-K]
    return int(np.sum(pos > kth))


def hits_at(pos, neg, K):
    """OGB's Hits@K."""
    c = hits_count(pos, neg, K)
    return 1.0 if c is None else c / _f32(pos).size


def mrr_list(pos, neg):
    """(mrr_list fp32 [P], rank fp32 [P]): rank = (#{neg > pos} + #{neg >= pos}) / 2 + 1, mrr = 1 / rank in fp32."""
    pos = _f32(pos)
    neg = np.asarray(neg, dtype=np.float32).reshape(pos.size, -1)
    opt = np.sum(neg > pos[:, None], axis=1).astype(np.float64)
    pes = np.sum(neg >= pos[:, None], axis=1).astype(np.float64)
    rank = (0.5 * (opt + pes) + 1.0).astype(np.float32)
    return (np.float32(1.0) / rank).astype(np.float32), rank


def mrr(pos, neg):
    """{'MRR': fp64 mean of the list, 'hits@1', 'hits@3', 'hits@10'}."""
    lst, rank = mrr_list(pos, neg)
    out = {"MRR": float(np.mean(lst.astype(np.float64)))}
    for j in (1, 3, 10):
        out[f"hits@{j}"] = float(np.mean(rank <= j))
    return out
