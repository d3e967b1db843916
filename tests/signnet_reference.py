"""One SIGNNet training step restated in numpy (reference models.py:301-383 and harness.SIGNNetTwin read, nothing
copied): operator_diff = Linear, ELU, BatchNorm (batch statistics over the rows of the batch), dropout; the centre pool;
link_pred_mlp = Linear, ReLU, BatchNorm over the links, dropout, Linear; BCE with logits (mean); the backward; dense Adam
in torch's operation order; both BatchNorms' running statistics.  Dropout masks and link ids are handed in.

A state is a dict: the ten tensors W1 [H, IW], b1, g1, be1, W2 [H, ch·H], b2, g2, be2, W3 [1, H], b3 [1]; "m" and "v",
dicts of Adam's moments under the same names; rm1, rv1, rm2, rv2 [H]; t (Adam's step count) and nbt
(num_batches_tracked).  The store is x [ΣR, IW] with row_ptr [L + 1]; a batch is a list of link ids; mask1 [ΣR_b, H] in
batch-row order and mask2 [B, H] hold 0 / 1 (None: all kept).  mode is "" (no pooled rows), "mean" or "sum".

`Sums(np.float32, rng)` runs the same arithmetic in fp32 with every sum's terms in a random order (a draw of the
rounding a kernel's own order could give); `Sums()` is fp64 in the natural order.  `fault=` restates one wrong kernel."""
import numpy as np

BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
NAMES = ("W1", "b1", "g1", "be1", "W2", "b2", "g2", "be2", "W3", "b3")
FAULTS = ("second_centre_row_of_next_link", "mean_over_all_rows_of_the_link", "bn1_statistics_over_the_links",
          "running_var_biased", "last_hidden_column_skipped", "last_row_tile_skipped", "one_mask_for_both_dropouts",
          "beta_gradients_dropped", "empty_link_pools_its_neighbours_rows")
ROW_TILE = 64


class Sums:
    """How sums are formed: the dtype of every operation and, with rng, a random order of every sum's terms."""

    def __init__(self, dtype=np.float64, rng=None):
        self.dtype, self.rng = dtype, rng

    def mm(self, a, b):
        """a [n, k] @ b [k, m]"""
        if self.rng is not None:
            perm = self.rng.permutation(a.shape[1])
            a, b = np.ascontiguousarray(a[:, perm]), np.ascontiguousarray(b[perm])
        return (a @ b).astype(self.dtype)

    def sum0(self, a):
        if self.rng is not None:
            a = a[self.rng.permutation(a.shape[0])]
        return a.sum(axis=0, dtype=self.dtype)


def new_state(params):
    st = {k: np.array(params[k], dtype=np.float64) for k in NAMES}
    H = st["b1"].shape[0]
    st["m"] = {k: np.zeros_like(st[k]) for k in NAMES}
    st["v"] = {k: np.zeros_like(st[k]) for k in NAMES}
    st.update(rm1=np.zeros(H), rv1=np.ones(H), rm2=np.zeros(H), rv2=np.ones(H), t=0, nbt=0)
    return st


def batch_rows(row_ptr, ids):
    """(store rows of the batch in batch order [R], local row_ptr [B + 1])"""
    row_ptr, ids = np.asarray(row_ptr), np.asarray(ids)
    cnt = row_ptr[ids + 1] - row_ptr[ids]
    lptr = np.concatenate([[0], np.cumsum(cnt)])
    ridx = np.concatenate([np.arange(row_ptr[i], row_ptr[i + 1]) for i in ids])
    return ridx, lptr


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0)))


def forward(st, X, lptr, mask1, mask2, p, mode, train, S=None, fault=None):
    """Everything the backward needs, as a dict; "logit" [B].  train=False: running statistics, no dropout."""
    S = S or Sums()
    dt = S.dtype
    P = {k: st[k].astype(dt) for k in NAMES}
    X = X.astype(dt)
    B, R, H = len(lptr) - 1, X.shape[0], P["b1"].shape[0]
    scale = dt(1.0 / (1.0 - p)) if train else dt(1)
    keep1 = np.ones((R, H), dt) if (mask1 is None or not train) else np.asarray(mask1, dtype=dt)
    keep2 = np.ones((B, H), dt) if (mask2 is None or not train) else np.asarray(mask2, dtype=dt)
    first = lptr[:-1]
    second = first + 1
    if fault == "second_centre_row_of_next_link":
        second = np.roll(first, -1) + 1
    if fault == "one_mask_for_both_dropouts":
        keep2 = keep1[first]
    pre = S.mm(X, P["W1"].T) + P["b1"]
    a = elu(pre).astype(dt)
    if train:
        stat_rows = a[first] if fault == "bn1_statistics_over_the_links" else a
        n1 = stat_rows.shape[0]
        mean1 = S.sum0(stat_rows) / dt(n1)
        var1 = S.sum0((stat_rows - mean1) ** 2) / dt(n1)
    else:
        n1, mean1, var1 = R, st["rm1"].astype(dt), st["rv1"].astype(dt)
    inv1 = (1 / np.sqrt(var1 + dt(BN_EPS))).astype(dt)
    xhat1 = (a - mean1) * inv1
    h = (xhat1 * P["g1"] + P["be1"]) * keep1 * scale
    if fault == "last_hidden_column_skipped":
        h = h.copy()
        h[:, -1] = 0
    z = h[first] * h[second]
    pool_rows, pool_scale = [], np.ones(B, dt)
    if mode:
        pooled = np.zeros((B, H), dt)
        for b in range(B):
            rows = np.arange(lptr[b] + 2, lptr[b + 1])
            if fault == "empty_link_pools_its_neighbours_rows" and not rows.size:
                nb = (b + 1) % B
                rows = np.arange(lptr[nb] + 2, lptr[nb + 1])
            if mode == "mean" and rows.size:
                div = lptr[b + 1] - lptr[b] if fault == "mean_over_all_rows_of_the_link" else rows.size
                pool_scale[b] = dt(1) / dt(div)
            pool_rows.append(rows)
            acc = np.zeros(H, dt)
            for r in rows:                      # the kernel's order: row after row
                acc = acc + h[r]
            pooled[b] = acc * pool_scale[b]
        z = np.concatenate([z, pooled], axis=1)
    pre2 = S.mm(z, P["W2"].T) + P["b2"]
    r2 = np.maximum(pre2, 0)
    if train:
        mean2 = S.sum0(r2) / dt(B)
        var2 = S.sum0((r2 - mean2) ** 2) / dt(B)
    else:
        mean2, var2 = st["rm2"].astype(dt), st["rv2"].astype(dt)
    inv2 = (1 / np.sqrt(var2 + dt(BN_EPS))).astype(dt)
    xhat2 = (r2 - mean2) * inv2
    d2 = (xhat2 * P["g2"] + P["be2"]) * keep2 * scale
    logit = S.mm(d2, P["W3"].T)[:, 0] + P["b3"][0]
    return dict(P=P, X=X, pre=pre, a=a, n1=n1, mean1=mean1, var1=var1, inv1=inv1, xhat1=xhat1, h=h, keep1=keep1,
                keep2=keep2, scale=scale, first=first, second=second, z=z, pool_rows=pool_rows, pool_scale=pool_scale,
                pre2=pre2, mean2=mean2, var2=var2, inv2=inv2, xhat2=xhat2, d2=d2, logit=logit.astype(dt))


def loss_and_grads(st, x, row_ptr, y, ids, mask1, mask2, p, mode, S=None, fault=None):
    """(loss, grads {name: array}, the forward's dict)"""
    S = S or Sums()
    dt = S.dtype
    ridx, lptr = batch_rows(row_ptr, ids)
    f = forward(st, np.asarray(x)[ridx], lptr, mask1, mask2, p, mode, True, S, fault)
    P, o = f["P"], f["logit"]
    B, R, H = len(ids), len(ridx), P["b1"].shape[0]
    yb = np.asarray(y, dtype=dt)[np.asarray(ids)]
    loss = (np.maximum(o, 0) - o * yb + np.log1p(np.exp(-np.abs(o)))).sum(dtype=dt) / dt(B)
    dl = ((1 / (1 + np.exp(-o)) - yb) / dt(B)).astype(dt)
    g = {"W3": S.mm(dl[None, :], f["d2"]), "b3": np.array([dl.sum(dtype=dt)])}
    dbn2 = dl[:, None] * P["W3"] * f["keep2"] * f["scale"]
    g["be2"] = S.sum0(dbn2)
    g["g2"] = S.sum0(dbn2 * f["xhat2"])
    dr = P["g2"] * f["inv2"] * (dbn2 - g["be2"] / dt(B) - f["xhat2"] * (g["g2"] / dt(B)))
    dpre2 = (dr * (f["pre2"] > 0)).astype(dt)
    g["b2"] = S.sum0(dpre2)
    g["W2"] = S.mm(dpre2.T, f["z"])
    dz = S.mm(dpre2, P["W2"])
    h, first, second = f["h"], f["first"], f["second"]
    dh = np.zeros((R, H), dt)
    np.add.at(dh, first, dz[:, :H] * h[second])
    np.add.at(dh, second, dz[:, :H] * h[first])
    if mode:
        for b, rows in enumerate(f["pool_rows"]):
            if rows.size:
                np.add.at(dh, rows, dz[b, H:] * f["pool_scale"][b])
    if fault == "last_hidden_column_skipped":
        dh[:, -1] = 0
    dbn1 = dh * f["keep1"] * f["scale"]
    n1 = dt(f["n1"])
    g["be1"] = S.sum0(dbn1)
    g["g1"] = S.sum0(dbn1 * f["xhat1"])
    if fault == "bn1_statistics_over_the_links":     # the adjoint of statistics that see only the first rows
        onstat = np.zeros((R, 1), dt)
        onstat[first] = 1
        sb, sg = S.sum0(dbn1), S.sum0(dbn1 * f["xhat1"])
        da = P["g1"] * f["inv1"] * (dbn1 - onstat * (sb / n1 + f["xhat1"] * (sg / n1)))
    else:
        da = P["g1"] * f["inv1"] * (dbn1 - g["be1"] / n1 - f["xhat1"] * (g["g1"] / n1))
    dpre = (da * np.where(f["pre"] > 0, dt(1), np.exp(np.minimum(f["pre"], 0)))).astype(dt)
    g["b1"] = S.sum0(dpre)
    rows_in = R if fault != "last_row_tile_skipped" else (R - 1) // ROW_TILE * ROW_TILE
    g["W1"] = S.mm(dpre[:rows_in].T, f["X"][:rows_in])
    if fault == "beta_gradients_dropped":
        g["be1"], g["be2"] = np.zeros_like(g["be1"]), np.zeros_like(g["be2"])
    return dt(loss), {k: np.asarray(g[k], dtype=dt).reshape(st[k].shape) for k in NAMES}, f


def adam(w, m, v, g, t, lr):
    """torch.optim.Adam's update number t (1-based) of one tensor: returns (w', m', v')."""
    m2 = m + (g - m) * (1 - BETA1)
    v2 = v * BETA2 + (1 - BETA2) * g * g
    bc1, bc2 = 1 - BETA1 ** t, 1 - BETA2 ** t
    return w - (lr / bc1) * (m2 / (np.sqrt(v2) / np.sqrt(bc2) + ADAM_EPS)), m2, v2


def running(f, B, fault=None):
    """The batch statistics both BatchNorms fold into their running ones: (mean1, var1 unbiased, mean2, var2 unbiased)"""
    n1 = f["n1"]
    u1 = 1.0 if fault == "running_var_biased" else n1 / (n1 - 1)
    u2 = 1.0 if fault == "running_var_biased" else B / (B - 1)
    return f["mean1"], f["var1"] * u1, f["mean2"], f["var2"] * u2


def apply(st, grads, stats, lr):
    """The state after Adam on fp64 copies of `grads` and the running-stat update with `stats`."""
    t = st["t"] + 1
    new = {"m": {}, "v": {}, "t": t, "nbt": st["nbt"] + 1}
    for k in NAMES:
        new[k], new["m"][k], new["v"][k] = adam(st[k], st["m"][k], st["v"][k], np.asarray(grads[k], np.float64), t, lr)
    for name, s in zip(("rm1", "rv1", "rm2", "rv2"), stats):
        new[name] = (1 - BN_MOMENTUM) * st[name] + BN_MOMENTUM * np.asarray(s, np.float64)
    return new


def step(st, x, row_ptr, y, ids, mask1, mask2, p, mode, lr, S=None, fault=None):
    """One optimiser step: (new state, loss, grads, forward dict)."""
    loss, grads, f = loss_and_grads(st, x, row_ptr, y, ids, mask1, mask2, p, mode, S, fault)
    return apply(st, grads, running(f, len(ids), fault), lr), float(loss), grads, f


def score(st, x, row_ptr, mode, S=None):
    """The logits of every link of the store in eval mode."""
    row_ptr = np.asarray(row_ptr)
    lptr = row_ptr - row_ptr[0]
    X = np.asarray(x)[row_ptr[0]:row_ptr[-1]]
    return forward(st, X, lptr, None, None, 0.0, mode, False, S)["logit"]
