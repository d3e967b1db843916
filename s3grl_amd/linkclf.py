"""The link classifier of the reference's N2V row (baselines/n2v.py: sklearn's default `LogisticRegression` over the
Hadamard features `emb[src] * emb[dst]`, then `clf.predict`), as HIP kernels behind the C ABI (s3grl_linkclf_*,
csrc/s3grl_linkclf.hip).

    clf = LinkClassifier(32); clf.fit(emb, pairs, labels); tp, fp, fn, tn = clf.confusion(emb, test_pairs, test_labels)
    auc, ap = hard_auc_ap(tp, fp, fn, tn)

What is computed is the minimiser over θ = (w, b) of sklearn's objective (penalty='l2', C, fit_intercept=True),

    f(θ) = ½ w·w + C Σ_i [ log(1 + exp(z_i)) − y_i z_i ],   z_i = (emb[src_i] ⊙ emb[dst_i])·w + b,

by damped Newton in fp64 from θ = 0 (step θ − t H⁻¹∇f, the first t of 1, ½, … 2⁻¹⁵ that meets Armijo with c₁ = 1e-4),
until max|∇f| <= tol.  sklearn's lbfgs stops at its own tol = 1e-4, a few 1e-3 away in the coefficients: `coef_` here is
what sklearn gives with `tol=1e-12, max_iter=100000`, not its default stopping point.  The table is read in place
through the pair list, on the device; no [M, D] feature matrix is formed and nothing comes to the host but θ.  Two fits
of one input are bit-identical.  GPU only; no CPU fallback.  fit_intercept=False, class weights, an L1 or multinomial
model and dim > 128 are not implemented.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np
import torch

from . import _native as N


class TableRef:
    """A live fp32 [num_nodes, dim] table on the device that some trainer owns (`Node2Vec._table()`): its address, not
    a copy.  `owner` is kept alive with it."""

    def __init__(self, ptr, num_nodes, dim, owner):
        self.ptr, self.num_nodes, self.dim, self.owner = int(ptr), int(num_nodes), int(dim), owner


def layout(dim):
    """The lane layout of the row kernels, without a GPU: dict(channels_per_lane, lanes_per_row, rows_per_block,
    max_blocks).  A row (one pair) is worked on by lanes_per_row lanes, each channels_per_lane channels; a workgroup
    takes rows_per_block rows, and past max_blocks workgroups several such tiles one after the other."""
    dim = _check_dim(dim)
    out = (ct.c_int32 * 4)()
    N.check(N.lib().s3grl_linkclf_layout(dim, out), "s3grl_linkclf_layout")
    return {"channels_per_lane": out[0], "lanes_per_row": out[1], "rows_per_block": out[2], "max_blocks": out[3]}


def _check_dim(dim):
    dim = int(dim)
    if not 1 <= dim <= N.LINKCLF_MAX_DIM:
        raise ValueError(f"dim must be in [1, {N.LINKCLF_MAX_DIM}], got {dim}")
    return dim


def hard_auc_ap(tp, fp, fn, tn):
    """(AUC, AP) of a 0/1 prediction vector from its confusion counts: what `heuristics.roc_auc` and
    `heuristics.average_precision` (sklearn's roc_auc_score and average_precision_score) give on the vector itself.
    With P = tp + fn positives and N = fp + tn negatives the ROC curve has the one inner point (fp/N, tp/P), so
    AUC = (TPR + TNR) / 2, the balanced accuracy, and AP = precision · recall + (1 − recall) · P / (P + N).  When every
    prediction is the same class the curve is the diagonal: AUC = 1/2 and AP = P / (P + N).  A label vector without a
    positive (AP, AUC) or without a negative (AUC) raises ValueError, as those two functions do."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    if min(tp, fp, fn, tn) < 0:
        raise ValueError("counts must be non-negative")
    pos, neg = tp + fn, fp + tn
    if pos == 0:
        raise ValueError("AP needs a positive in y_true")
    if neg == 0:
        raise ValueError("AUC needs both classes in y_true")
    prevalence = pos / (pos + neg)
    if tp + fp == 0 or fn + tn == 0:          # one threshold only
        return 0.5, prevalence
    recall = tp / pos
    return (recall + tn / neg) / 2.0, tp / (tp + fp) * recall + (1.0 - recall) * prevalence


class LinkClassifier:
    """sklearn `LogisticRegression(C=C)` over emb[src] ⊙ emb[dst], solved to max|∇f| <= tol on the device."""

    def __init__(self, dim, C=1.0, tol=1e-8, max_iter=50, device=None, *, fit_intercept=True):
        if not fit_intercept:
            raise NotImplementedError("LinkClassifier with fit_intercept=False: the reference fits the intercept")
        self.dim = _check_dim(dim)
        self.C, self.tol, self.max_iter = float(C), float(tol), int(max_iter)
        if not self.C > 0 or not np.isfinite(self.C):
            raise ValueError(f"C must be positive and finite, got {C}")
        if not self.tol >= 0:
            raise ValueError(f"tol must be non-negative, got {tol}")
        if not 0 <= self.max_iter <= 10000:
            raise ValueError(f"max_iter must be in [0, 10000], got {max_iter}")
        if device is not None and torch.device(device).type == "cpu":
            raise RuntimeError("the link classifier needs a HIP device (MI355X); there is no CPU fallback")
        from .engine import default_engine

        self.engine = default_engine(device)
        h = ct.c_void_p()
        N.check(N.lib().s3grl_linkclf_create(self.engine._ctx, self.dim, self.C, self.tol, self.max_iter, ct.byref(h)),
                "s3grl_linkclf_create")
        self._h = h
        self._state = None
        self.engine._children.add(self)   # the engine closes it before its context goes

    # -- arguments --------------------------------------------------------------------------------------------
    def _table(self, emb):
        """emb -> (device address, num_nodes, what to keep alive while the launches run)."""
        if isinstance(emb, TableRef):
            if emb.dim != self.dim:
                raise ValueError(f"emb must be [N, {self.dim}], got [{emb.num_nodes}, {emb.dim}]")
            return ct.c_void_p(emb.ptr), emb.num_nodes, emb
        t = torch.as_tensor(emb)
        if t.dim() != 2 or t.shape[1] != self.dim or not t.shape[0]:
            raise ValueError(f"emb must be [N, {self.dim}], got {tuple(t.shape)}")
        t = t.to(device=self.engine.device, dtype=torch.float32).contiguous()
        return N.ptr(t), t.shape[0], t

    def _rows(self, pairs, num_nodes, labels=None, empty_ok=False):
        from .mf import _pairs

        p = _pairs(pairs, num_nodes, "pairs", empty_ok=empty_ok)
        dev = self.engine.device
        y = None
        if labels is not None:
            y = torch.as_tensor(labels).reshape(-1)
            if y.shape[0] != p.shape[0]:
                raise ValueError(f"need one label per pair, got {y.shape[0]} for {p.shape[0]}")
            y = (y != 0).to(device=dev, dtype=torch.uint8).contiguous()
        return p.to(device=dev, dtype=torch.int32).contiguous(), y

    @staticmethod
    def _two_classes(y):
        ones = int(y.sum())
        if ones == 0 or ones == y.shape[0]:
            raise ValueError("This solver needs samples of at least 2 classes in the data, but the data contains only "
                             f"one class: {1 if ones else 0}")

    # -- fitting ----------------------------------------------------------------------------------------------
    def fit(self, emb, pairs, labels, init=None):
        """The minimiser for pairs [M, 2] (node ids) with labels [M] (non-zero: a link), from θ = 0 or from init fp64
        [dim + 1] (w, then b).  One wait for the argument check, then max_iter × 4 launches and one read of the
        state.  Returns self."""
        self._alive()
        e, n, keep = self._table(emb)
        p, y = self._rows(pairs, n, labels)
        self._two_classes(y)
        th0 = None
        if init is not None:
            th0 = np.ascontiguousarray(np.asarray(init, dtype=np.float64).reshape(-1))
            if th0.shape[0] != self.dim + 1 or not np.isfinite(th0).all():
                raise ValueError(f"init must be {self.dim + 1} finite values (w, then b)")
        N.check(N.lib().s3grl_linkclf_fit(self._h, e, n, N.ptr(p), N.ptr(y), p.shape[0],
                                          None if th0 is None else th0.ctypes.data_as(ct.c_void_p)),
                "s3grl_linkclf_fit")
        self._read()
        del keep
        if self._state["done"] == 3:
            raise RuntimeError(f"the Newton iteration stopped: {N.LINKCLF_DONE[3]} (a non-finite table?)")
        return self

    def newton_step(self, emb, pairs, labels):
        """One Newton iteration from the current θ (0 before any fit); returns the state after it.  The
        teacher-forcing hook: it runs the four launches an iteration of `fit` runs."""
        self._alive()
        e, n, keep = self._table(emb)
        p, y = self._rows(pairs, n, labels)
        self._two_classes(y)
        N.check(N.lib().s3grl_linkclf_newton_step(self._h, e, n, N.ptr(p), N.ptr(y), p.shape[0]),
                "s3grl_linkclf_newton_step")
        del keep
        return self._read()

    def _read(self):
        n = self.dim + 1
        theta, grad = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
        loss, step_t, n_iter, done = ct.c_double(), ct.c_double(), ct.c_int32(), ct.c_int32()
        N.check(N.lib().s3grl_linkclf_state(self._h, theta.ctypes.data_as(ct.c_void_p), grad.ctypes.data_as(ct.c_void_p),
                                            ct.byref(loss), ct.byref(step_t), ct.byref(n_iter), ct.byref(done)),
                "s3grl_linkclf_state")
        self._state = {"theta": theta, "grad": grad, "loss": loss.value, "step_t": step_t.value,
                       "n_iter": n_iter.value, "done": done.value}
        return self._state

    def state(self):
        """dict(theta fp64 [dim + 1] the current θ; grad, loss: ∇f and f where the last iteration began; step_t the t
        it took (0: none); n_iter the steps taken; done 0: not yet, 1: max|∇f| <= tol at θ, 2 / 3: stopped)."""
        self._alive()
        return self._read()

    def _fitted(self):
        if self._state is None:
            raise RuntimeError("this LinkClassifier is not fitted yet")
        return self._state

    @property
    def coef_(self):
        return self._fitted()["theta"][None, :-1].copy()

    @property
    def intercept_(self):
        return self._fitted()["theta"][-1:].copy()

    @property
    def n_iter_(self):
        return self._fitted()["n_iter"]

    @property
    def converged_(self):
        return self._fitted()["done"] == 1

    # -- prediction -------------------------------------------------------------------------------------------
    def _predict(self, emb, pairs, labels, decision, counts):
        self._alive()
        self._fitted()
        e, n, keep = self._table(emb)
        p, y = self._rows(pairs, n, labels, empty_ok=True)
        dev, M = self.engine.device, p.shape[0]
        pred = torch.empty(M, dtype=torch.uint8, device=dev)
        dec = torch.empty(M, dtype=torch.float32, device=dev) if decision else None
        cnt = torch.empty(4, dtype=torch.int64, device=dev) if counts else None
        N.check(N.lib().s3grl_linkclf_predict(self._h, e, n, N.ptr(p), M, N.ptr(y), N.ptr(pred), N.ptr(dec),
                                              N.ptr(cnt)), "s3grl_linkclf_predict")
        del keep
        return pred, dec, cnt

    def predict(self, emb, pairs):
        """`clf.predict`: uint8 [M] on the device, 1 where z > 0."""
        return self._predict(emb, pairs, None, False, False)[0]

    def decision_function(self, emb, pairs):
        """`clf.decision_function`: z as fp32 [M] on the device."""
        return self._predict(emb, pairs, None, True, False)[1]

    def confusion(self, emb, pairs, labels):
        """(tp, fp, fn, tn) of `predict` against labels [M], counted on the device."""
        return tuple(int(v) for v in self._predict(emb, pairs, labels, False, True)[2].cpu())

    def _alive(self):
        if getattr(self, "_h", None) is None:
            raise RuntimeError("LinkClassifier is closed")

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and self.engine._ctx:   # it works on the context's stream
            N.lib().s3grl_linkclf_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
