"""What the node2vec GPU tests share (tests/test_gpu_node2vec.py, tests/test_gpu_node2vec_shapes.py) and what the host
tests check of it (tests/test_node2vec_host.py): the window contract, the per-element bounds of one teacher-forced step
against the fp64 restatement (tests/node2vec_reference.py), the lane-layout rule of csrc/s3grl_node2vec.hip restated,
and a row's gradient terms in the order the engine's sort puts them, so a test can restate a wrong kernel.  numpy and
torch only; nothing here needs a GPU until a trainer object is passed in."""
import numpy as np
import torch

from node2vec_reference import EPS, loss_and_grad, windows_of
from node2vec_reference import step as ref_step


# ---- the windows the engine draws ----------------------------------------------------------------------------------
def walks_of(win, rows, C, W):
    """Walk rows back from window-major windows: window 0 of every row, then the last node of windows 1..W-1."""
    w = win.reshape(W, rows, C)
    return np.concatenate([w[0], w[1:, :, C - 1].T], axis=1)


def check_windows(n2v, ei, N, epoch, bs=32):
    from s3grl_amd.node2vec import csr_of

    ip, ix = csr_of(ei, N)
    R, Q, C, L = n2v.walks_per_node, n2v.num_negative_samples, n2v.context_size, n2v.walk_length
    W = L + 2 - C
    batches = []
    for s in range(n2v.steps_per_epoch(bs)):
        pos, neg = (x.cpu().numpy() for x in n2v.windows(epoch, s, bs))
        B = min(bs, N - s * bs)
        batch = pos[:B, 0]
        batches.append(batch)
        assert pos.shape == (W * B * R, C) and neg.shape == (W * B * R * Q, C)
        rw = walks_of(pos, B * R, C, W)
        assert np.array_equal(rw[:, 0], np.tile(batch, R))                 # batch.repeat(walks_per_node)
        assert np.array_equal(windows_of(rw, C), pos)                      # window-index-major
        a, b = rw[:, :-1].reshape(-1), rw[:, 1:].reshape(-1)
        for u, v in zip(a, b):                                             # a CSR entry, or a stay at a sink
            row = ix[ip[u]:ip[u + 1]]
            assert (v in row) if len(row) else v == u
        nw = walks_of(neg, B * R * Q, C, W)
        assert np.array_equal(nw[:, 0], np.tile(batch, R * Q))
        assert np.array_equal(windows_of(nw, C), neg)
        assert nw.min() >= 0 and nw.max() < N
    perm = np.concatenate(batches)
    assert np.array_equal(np.sort(perm), np.arange(N))                     # the epoch is a permutation
    return perm


# ---- one teacher-forced step against the restatement ---------------------------------------------------------------
def tolerances(h, m, v, t, pos, neg, lr):
    """Per-element bounds of |engine - fp64 restatement| for one step from the same fp32 state.
    g: the engine forms each dot in fp32 (<= D products) and sums a row's terms g·h in fp32, a few thousand for a hub
    row; the rounding error of such sums is taken as 1e-5 · Σ|g·h| (sqrt(k) · 6e-8 with k <= 4 400 is 4e-6, and each
    g carries the fp32 error of its dot, ~1e-6 relative, through the sigmoid derivative).  m' = m + 0.1 (g - m) and
    v' = v + 0.001 (g² - v) carry it scaled; h' = h - s · m'/(sqrt(v') + eps) carries it through the first-order
    sensitivity to m' and v'.  Every quantity also gets 4 fp32 ulps of its own rounding."""
    _, grad, _ = loss_and_grad(h, pos, neg, fp32_sigmoid=True)
    _, gabs, _ = loss_and_grad(h, pos, neg, magnitude=True, fp32_sigmoid=True)
    tg = 1e-5 * gabs
    ulp = 4 * 2.0 ** -23
    m2 = m + (grad - m) * 0.1
    v2 = v + (grad * grad - v) * 0.001
    tm = 0.1 * tg + ulp * np.abs(m2) + 1e-30
    tv = 0.001 * 2 * np.abs(grad) * tg + 0.001 * tg * tg + ulp * np.abs(v2) + 1e-36
    ss = lr * np.sqrt(1 - 0.999 ** (t + 1)) / (1 - 0.9 ** (t + 1))
    sv = np.sqrt(v2)
    upd = ss * np.abs(m2) / (sv + 1e-8)
    th = ss * tm / (sv + 1e-8) + upd * tv / (2 * np.maximum(v2, 1e-60)) + ulp * (np.abs(h) + upd)
    return tm, tv, np.minimum(th, 2 * ss)   # a step moves an element by at most about s: 2 s bounds any error


def dots_of(h, win):
    """<h[w0], h[wi]> of every window, [P, C-1]."""
    return np.einsum("pd,pcd->pc", h[win[:, 0]], h[win[:, 1:]])


def step_check(n2v, pos, neg, lr, worst, tag, saturated_past=np.inf, before_step=None):
    """One `n2v.step(pos, neg, lr)` against the restatement's step from the same state, within `tolerances`; updates
    worst = [h, m, v error / bound, loss relative error] in place.  before_step(h, pos, neg) sees the fp64 copy of
    the state first.  saturated_past: the caller has asserted that no negative dot lies just below it and that every
    one above it is saturated in fp32 on either side, so those keep the 1e-5 loss tolerance."""
    st = n2v.state()
    h, m, v = (st[k].cpu().double().numpy() for k in ("weight", "exp_avg", "exp_avg_sq"))
    pos, neg = (np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x) for x in (pos, neg))
    if before_step is not None:
        before_step(h, pos, neg)
    hr, mr, vr, lr_loss = ref_step(h, m, v, st["step"], pos, neg, lr, fp32_sigmoid=True)
    # loss: 1e-5 relative for fp32 dots and logs, plus, for every negative dot within 2^-18 of saturation
    # (1 - s a few fp32 steps of 2^-24 from 0), the most its term -log(1 - s + EPS) can move when the
    # engine's fp32 dot lands one step of s away: log(2^-24 / EPS) < 18, over that mean's n
    out_neg = dots_of(h, neg)
    near = int(((out_neg > 12.4) & (out_neg <= saturated_past)).sum())          # 1 - sigmoid(12.4) ~ 2^-18
    tl = 1e-5 * abs(lr_loss) + 18.0 * near / out_neg.size
    tm, tv, th = tolerances(h, m, v, st["step"], pos, neg, lr)
    loss = n2v.step(pos, neg, lr)
    st2 = n2v.state()
    assert st2["step"] == st["step"] + 1
    hg, mg, vg = (st2[k].cpu().double().numpy() for k in ("weight", "exp_avg", "exp_avg_sq"))
    for i, (got, ref, tol) in enumerate(((hg, hr, th), (mg, mr, tm), (vg, vr, tv))):
        r = np.abs(got - ref) / tol
        worst[i] = max(worst[i], float(r.max()))
        if not r.max() <= 1.0:
            u, c = np.unravel_index(int(np.nan_to_num(r, nan=np.inf).argmax()), r.shape)
            uses = int((pos == u).sum() + (neg == u).sum())
            raise AssertionError(f"{'hmv'[i]} {tag}: row {u} col {c} ({uses} window slots) "
                                 f"engine {got[u, c]!r} ref {ref[u, c]!r} tol {tol[u, c]!r}; before h "
                                 f"{h[u, c]!r} m {m[u, c]!r} v {v[u, c]!r}; m engine {mg[u, c]!r} ref "
                                 f"{mr[u, c]!r} tol {tm[u, c]!r}")
    assert abs(loss - lr_loss) <= tl, (loss, lr_loss, tl)
    worst[3] = max(worst[3], abs(loss - lr_loss) / abs(lr_loss))
    return loss, lr_loss


def parity(n2v, steps, bs=32, lr=0.01, before_step=None):
    worst = [0.0, 0.0, 0.0, 0.0]
    done = 0
    e = 0
    while done < steps:
        for s in range(n2v.steps_per_epoch(bs)):
            if done == steps:
                break
            pos, neg = n2v.windows(e, s, bs)
            step_check(n2v, pos, neg, lr, worst, f"epoch {e} step {s}", before_step=before_step)
            done += 1
        e += 1
    return worst


def same_state(a, b):
    sa, sb = a.state(), b.state()
    return sa["step"] == sb["step"] and all(torch.equal(sa[k], sb[k]) for k in ("weight", "exp_avg", "exp_avg_sq"))


# ---- the lane layouts of s3grl_node2vec.hip ------------------------------------------------------------------------
def lanes_rule(D):
    """s3grl_skipgram_create's choice restated: (VEC, LPD, trips of the channel loop).  VEC = 4 when D % 4 == 0, LPD the
    smallest power of two >= D / VEC, at most 64."""
    vec = 4 if D % 4 == 0 else 1
    lpd = 1
    while lpd < D // vec and lpd < 64:
        lpd *= 2
    return vec, lpd, -(-D // (lpd * vec))


# D -> (VEC, LPD, trips): the table of tests/test_gpu_gae_shapes.py, whose kernels choose their lanes by the same rule
DIMS = {
    1: (1, 1, 1), 2: (1, 2, 1), 3: (1, 4, 1), 5: (1, 8, 1), 13: (1, 16, 1), 17: (1, 32, 1), 33: (1, 64, 1),
    65: (1, 64, 2),
    4: (4, 1, 1), 8: (4, 2, 1), 12: (4, 4, 1), 16: (4, 4, 1), 20: (4, 8, 1), 64: (4, 16, 1), 128: (4, 32, 1),
    256: (4, 64, 1), 260: (4, 64, 2), 512: (4, 64, 2), 1000: (4, 64, 4), 1028: (4, 64, 5),
}


# ---- the hub graph and its init table ------------------------------------------------------------------------------
HUB_N = 70
HUB_CFG = dict(walk_length=6, context_size=3, walks_per_node=2, num_negative_samples=1)
HUB_BS = 16


def hub_graph(n=HUB_N, seed=7):
    """Node 0 is a hub: every node 1..n-3 has an arc to it and one from it, and one arc to another of 1..n-3, so
    every second step of a walk is the hub.  Node n-2 has in-arcs only (a sink); node n-1 has no edges."""
    rng = np.random.default_rng(seed)
    x = np.arange(1, n - 2)
    other = rng.choice(x, len(x))
    src = np.concatenate([x, np.zeros(len(x), dtype=np.int64), x, x[:5]])
    dst = np.concatenate([np.zeros(len(x), dtype=np.int64), x, other, np.full(5, n - 2)])
    return np.stack([src, dst]), n


def init_table(n, D, seed, c=1.5, cap=6.0):
    """fp32 N(0, 1) · c / sqrt(D): self-dots about c², other dots about c² / sqrt(D), so no sigmoid is saturated at
    any D; scaled down when a dot of any two rows passes `cap`."""
    h = np.random.default_rng(seed).standard_normal((n, D)) * c / np.sqrt(D)
    worst = float(np.abs(h @ h.T).max())
    if worst > cap:
        h *= np.sqrt(cap / worst)
    return torch.as_tensor(h, dtype=torch.float32)


def row_uses(pos, neg, u):
    """The number of gradient terms row u collects in one step: one per dot it starts, one per dot it is the context
    of (a self-dot counts twice)."""
    return sum(int((w[:, 0] == u).sum()) * (w.shape[1] - 1) + int((w[:, 1:] == u).sum())
               for w in (np.asarray(pos), np.asarray(neg)))


def host_windows(ei, n, batch, rng, walk_length, context_size, walks_per_node, num_negative_samples):
    """Windows with the engine's contract, drawn by numpy: for the host tests, which have no engine to draw them."""
    from s3grl_amd.node2vec import csr_of

    ip, ix = csr_of(ei, n)
    start = np.tile(np.asarray(batch), walks_per_node)
    rw = np.empty((len(start), walk_length + 1), dtype=np.int64)
    rw[:, 0] = start
    for s in range(1, walk_length + 1):
        for r, u in enumerate(rw[:, s - 1]):
            deg = ip[u + 1] - ip[u]
            rw[r, s] = ix[ip[u] + rng.integers(deg)] if deg else u
    nstart = np.tile(np.asarray(batch), walks_per_node * num_negative_samples)
    nw = np.concatenate([nstart[:, None], rng.integers(0, n, (len(nstart), walk_length))], axis=1)
    return windows_of(rw, context_size), windows_of(nw, context_size)


# ---- a row's terms as the engine orders them -----------------------------------------------------------------------
def dot_terms(h, pos, neg):
    """(start, other, g) per dot in the engine's dot order: positive windows then negative, window-major, context
    column minor; g is the loss derivative of the dot with sigmoid in fp32, as loss_and_grad(fp32_sigmoid=True)."""
    starts, others, gs = [], [], []
    for win, sign in ((np.asarray(pos), 1), (np.asarray(neg), -1)):
        out = dots_of(h, win)
        with np.errstate(over="ignore"):
            s = (np.float32(1) / (np.float32(1) + np.exp(-out).astype(np.float32))).astype(np.float64)
        g = -s * (1 - s) / (s + EPS) if sign > 0 else s * (1 - s) / (1 - s + EPS)
        starts.append(np.repeat(win[:, 0], win.shape[1] - 1))
        others.append(win[:, 1:].reshape(-1))
        gs.append(g.reshape(-1) / out.size)
    return np.concatenate(starts), np.concatenate(others), np.concatenate(gs)


def row_terms(h, pos, neg, u):
    """[k, D]: the terms g · h[other] of row u's gradient in the order of its sorted keys 2·dot + side (side 0: u
    starts the dot, side 1: u is its context).  row_grad_kernel's slice s of S sums terms s, s + S, ..."""
    start, other, g = dot_terms(h, pos, neg)
    a, b = np.flatnonzero(start == u), np.flatnonzero(other == u)
    key = np.concatenate([2 * a, 2 * b + 1])
    src = np.concatenate([other[a], start[b]])
    gg = np.concatenate([g[a], g[b]])
    o = np.argsort(key)
    return gg[o, None] * h[src[o]]
