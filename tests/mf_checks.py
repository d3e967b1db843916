"""What the MF tests share (tests/test_mf_host.py, tests/test_gpu_mf.py, tests/test_gpu_mf_shapes.py): the per-element
bounds of one teacher-forced step against the fp64 restatement (tests/mf_reference.py), derived from Σ|terms| of every
sum the engine forms in fp32; the shape list of the GPU parity test; the hub pair lists; and the restatement with one
fault each, so that a host test can show every fault lands far outside the bounds.  numpy and torch only; nothing here
needs a GPU until a trainer object is passed in."""
import numpy as np
import torch

import mf_reference as R

U = 2.0 ** -24          # fp32 unit roundoff
ULP = 4 * 2.0 ** -23    # every stored quantity's own rounding, 4 ulps as in node2vec_checks


# ---- shapes --------------------------------------------------------------------------------------------------------
# (H, num_layers, B) of the teacher-forced parity test.  H covers every (channels per lane, lanes per pair): 1, 2, 3
# (a non-multiple of 4), 7, 13, 32, 33 and 128; B covers 1, 5, 32, 33, one more than a tile (TILE_PLUS_1 resolves per
# H) and 1024; num_layers 2, 3, 4.
TILE_PLUS_1 = -1
SHAPES = [(1, 3, 33), (2, 2, 5), (3, 3, 33), (7, 4, 32), (13, 2, TILE_PLUS_1), (13, 3, 1), (13, 4, 33),
          (32, 3, 32), (32, 3, TILE_PLUS_1), (32, 2, 1024), (33, 3, 33), (33, 4, 5), (128, 3, 33), (128, 4, TILE_PLUS_1),
          (128, 2, 1), (32, 4, 1)]
LAYOUTS = {(1, 1, 256), (1, 2, 128), (1, 4, 64), (1, 8, 32), (1, 16, 16), (1, 32, 16), (1, 64, 16), (2, 64, 16)}


def resolve(shape, layout):
    H, L, B = shape
    return (H, L, layout(H, L, 1)["pairs_per_tile"] + 1) if B == TILE_PLUS_1 else shape


# ---- inputs --------------------------------------------------------------------------------------------------------
HUB_N = 70


def hub_pairs(B, rng, n=HUB_N):
    """(pos, neg) [B, 2] each over n nodes: node 0 is an endpoint of three pairs in four, as a and as b; from 2 pairs
    on one is a self-pair (5, 5), from 4 on one pair is listed twice; node n - 1 is in no pair."""
    p = rng.integers(1, n - 1, size=(2 * B, 2))
    i = np.arange(2 * B)
    p[i % 4 == 0, 0] = 0
    p[i % 4 == 1, 1] = 0
    p[i % 4 == 2, 0] = 0
    if B == 1:
        p[0] = (0, 0)
    if 2 * B >= 4:
        p[3] = (5, 5)
    if 2 * B >= 8:
        p[7] = p[6]
    return p[:B].copy(), p[B:].copy()


def init_params(n, H, L, seed, table_scale=1.0):
    """fp32 (table, layers): N(0, 1) · table_scale and torch's Linear default, uniform in ±1/sqrt(H)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, H)) * table_scale).astype(np.float32)
    b = 1 / np.sqrt(H)
    layers = []
    for l in range(L):
        out = 1 if l == L - 1 else H
        layers.append((rng.uniform(-b, b, (out, H)).astype(np.float32), rng.uniform(-b, b, out).astype(np.float32)))
    return x, layers


def random_masks(B, L, H, p, rng):
    return (rng.random((2 * B, L - 1, H)) >= p).astype(np.uint8)


# hand-built saturation: outputs of +18 (past the fp32 saturation of 1 - sigmoid), -18, 0 and -100
def saturated_params(H=4):
    """Hand-built weights: out = 18 · h0[0] - 100 · h0[1] through one identity-like hidden layer."""
    x = np.zeros((6, H), dtype=np.float32)
    x[0] = 1.0                                  # pairs with node 0 pick the other row
    x[1, 0] = 1.0                               # out = +18
    x[2, 0] = -1.0                              # hidden pre < 0 -> relu 0 -> out = bias
    x[3, 1] = 1.0                               # out = -100
    x[4, 0], x[4, 2] = 0.5, 1.0                 # out = 9 - 27 = -18
    W0 = np.eye(H, dtype=np.float32)
    w1 = np.zeros((1, H), dtype=np.float32)
    w1[0, 0], w1[0, 1], w1[0, 2] = 18.0, -100.0, -27.0
    return x, [(W0, np.zeros(H, dtype=np.float32)), (w1, np.zeros(1, dtype=np.float32))]


SATURATED_POS = np.array([[0, 1], [0, 3], [0, 4], [0, 2]])      # out 18, -100, -18, 0
SATURATED_NEG = np.array([[0, 1], [0, 3], [0, 4], [1, 1]])      # out 18 (1 - s = 0), -100, -18, 18


def state_of(mf):
    """The engine's state as a restatement state (fp64 copies)."""
    s = mf.state()

    def f(t):
        return t.cpu().double().numpy()

    def pairs(k):
        return [(f(W), f(b)) for W, b in s[k]]

    return {"x": f(s["weight"]), "xm": f(s["exp_avg"]), "xv": f(s["exp_avg_sq"]), "layers": pairs("layers"),
            "lm": pairs("layers_exp_avg"), "lv": pairs("layers_exp_avg_sq"), "t": s["step"]}


# ---- bounds --------------------------------------------------------------------------------------------------------
SATURATION = 16.6355      # fp32: 1 + exp(-out) rounds to 1 from here on, so 1 - sigmoid(out) is exactly 0


def grad_bounds(st, pos, neg, masks, p):
    """(gx, glayers, e_gx, e_glayers, e_loss, loss): the restatement's gradients with fp32 sigmoid and a bound on what
    an fp32 evaluation of the same sums may differ by.  A sum of k fp32 terms carries at most (k + 1) · U · Σ|terms|
    of rounding; errors of the inputs go through |W|; relu and dropout scale them by at most 1 / (1 - p).  Where a
    hidden pre-activation lies within its own bound of 0 the engine may take the other side of relu: the value moves
    by no more than the bound, but the derivative flips, so the whole incoming gradient is allowed there."""
    x, layers = st["x"], st["layers"]
    loss, (ga, gb), glayers, aux = R.loss_and_grads(x, layers, pos, neg, masks, p, fp32_sigmoid=True)
    acts, pres, dpres, pairs = aux["acts"], aux["pres"], aux["dpres"], aux["pairs"]
    L, H, B = len(layers), x.shape[1], len(pos)
    scale = 1.0 / (1.0 - p)
    keep = [np.ones_like(pres[0]) if masks is None else masks[:, l, :].astype(np.float64) for l in range(L - 1)]
    e_act, near = [U * np.abs(acts[0])], []
    for l in range(L - 1):
        W, b = layers[l]
        mag = np.abs(acts[l]) @ np.abs(W).T + np.abs(b)
        e_pre = e_act[l] @ np.abs(W).T + (H + 1) * U * mag
        near.append(np.abs(pres[l]) < e_pre)
        e_act.append(scale * keep[l] * (e_pre + U * np.abs(pres[l])))
    w, b = layers[-1]
    e_out = e_act[-1] @ np.abs(w[0]) + (H + 2) * U * (np.abs(acts[-1]) @ np.abs(w[0]) + np.abs(b[0]))
    out = aux["out"]
    # the loss: |d term / d out| <= 1, fp32 log and sigmoid a few ulps; a negative whose 1 - s is a few steps of 2^-24
    # from 0 may land one step away, which moves -log(1 - s + EPS) by up to log(2^-24 / EPS) < 18 (node2vec §10)
    close = int(((out[B:] > 12.4) & (out[B:] < SATURATION + 0.3)).sum())
    e_loss = e_out[:B].mean() + e_out[B:].mean() + 16 * U * (1 + abs(loss)) + 18.0 * close / B
    e_d = ((0.25 * e_out + 8 * U) / B + 4 * U * np.abs(aux["g"]))[:, None]
    e_gl = [None] * L
    for l in range(L - 1, -1, -1):
        W, _ = layers[l]
        d = np.abs(dpres[l])
        e_gW = e_d.T @ np.abs(acts[l]) + d.T @ e_act[l] + (2 * B + 2) * U * (d.T @ np.abs(acts[l]))
        e_gb = e_d.sum(axis=0) + (2 * B + 1) * U * d.sum(axis=0)
        e_gl[l] = (e_gW, e_gb)
        din = d @ np.abs(W)
        e_din = e_d @ np.abs(W) + (H + 1) * U * din
        if l > 0:
            on = (pres[l - 1] > 0) | near[l - 1]
            e_d = scale * keep[l - 1] * (on * (e_din + U * din) + near[l - 1] * np.abs(dpres[l] @ W))
        else:
            e_d = e_din
    e_ga = e_d * np.abs(x[pairs[:, 1]]) + U * np.abs(ga)
    e_gb = e_d * np.abs(x[pairs[:, 0]]) + U * np.abs(gb)
    n = len(x)
    gx = R.table_grad(n, pairs, ga, gb)
    e_gx = R.table_grad(n, pairs, e_ga, e_gb)
    count = np.bincount(pairs.reshape(-1), minlength=n)[:, None]
    e_gx += (count + 1) * U * R.table_grad(n, pairs, np.abs(ga), np.abs(gb))
    return gx, glayers, e_gx, e_gl, e_loss, loss


def adam_bounds(w, m, v, g, tg, t, lr):
    """Bounds (tw, tm, tv) of Adam update number t from the same (w, m, v) with gradients that differ by up to tg:
    m' and v' carry it scaled, w' through the first-order sensitivity to m' and to sqrt(v'); every quantity gets 4 fp32
    ulps of its own.  An update is at most 7.3 · ss · sqrt(bc2) in size ((1 - b1) / sqrt(1 - b2) · (1 - b1² / b2)^-½ by
    Cauchy-Schwarz over the history), so twice that bounds any error."""
    _, m2, v2 = R.adam(w, m, v, g, t, lr)
    tm = 0.1 * tg + ULP * np.abs(m2) + 1e-30
    tv = 0.001 * (2 * np.abs(g) * tg + tg * tg) + ULP * np.abs(v2) + 1e-36
    bc1, bc2 = 1 - R.BETA1 ** t, 1 - R.BETA2 ** t
    ss, sv = lr / bc1, np.sqrt(v2)
    denom = sv / np.sqrt(bc2) + R.ADAM_EPS
    upd = ss * np.abs(m2) / denom
    d_sqrt = np.minimum(tv / (2 * sv + 1e-300), np.sqrt(tv)) / np.sqrt(bc2)
    tw = ss * tm / denom + upd * d_sqrt / denom + ULP * (np.abs(w) + upd)
    return np.minimum(tw, 2 * 7.3 * ss * np.sqrt(bc2) + ULP * np.abs(w)), tm, tv


def step_bounds(st, pos, neg, masks, p, lr):
    """(the restatement's next state, loss, bounds): bounds mirrors the state's x / xm / xv / layers / lm / lv."""
    gx, glayers, e_gx, e_gl, e_loss, loss = grad_bounds(st, pos, neg, masks, p)
    new = R.apply_grads(st, gx, glayers, lr)
    t = st["t"] + 1
    b = {"layers": [], "lm": [], "lv": [], "loss": e_loss}
    b["x"], b["xm"], b["xv"] = adam_bounds(st["x"], st["xm"], st["xv"], gx, e_gx, t, lr)
    for (W, bi), (mW, mb), (vW, vb), (gW, gb), (eW, eb) in zip(st["layers"], st["lm"], st["lv"], glayers, e_gl):
        tw = adam_bounds(W, mW, vW, gW, eW, t, lr)
        tb = adam_bounds(bi, mb, vb, gb, eb, t, lr)
        for k, i in (("layers", 0), ("lm", 1), ("lv", 2)):
            b[k].append((tw[i], tb[i]))
    return new, loss, b


def worst_ratio(got, ref, bounds):
    """{name: max |got - ref| / bound} over the table, its moments and every layer's."""
    out = {}
    for k in ("x", "xm", "xv"):
        out[k] = float(np.max(np.abs(got[k] - ref[k]) / bounds[k]))
    for k in ("layers", "lm", "lv"):
        out[k] = max(float(np.max(np.abs(g - r) / b)) for gl, rl, bl in zip(got[k], ref[k], bounds[k])
                     for g, r, b in zip(gl, rl, bl))
    return out


def step_check(mf, pos, neg, masks, p, worst, tag):
    """One `mf.step(pos, neg, masks)` against the restatement's step from the same state, inside step_bounds; updates
    worst {name: ratio} in place and returns (engine loss, restatement loss)."""
    st = state_of(mf)
    ref, ref_loss, b = step_bounds(st, pos, neg, masks, p, mf.lr)
    loss = mf.step(torch.as_tensor(pos), torch.as_tensor(neg), None if masks is None else torch.as_tensor(masks))
    got = state_of(mf)
    assert got["t"] == st["t"] + 1
    r = worst_ratio(got, ref, b)
    r["loss"] = abs(loss - ref_loss) / b["loss"]
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{tag}: |engine - restatement| / bound = {bad} (loss {loss!r} vs {ref_loss!r})"
    assert np.isfinite(loss)
    return loss, ref_loss


def same_state(a, b):
    sa, sb = a.state(), b.state()
    if sa["step"] != sb["step"]:
        return False
    flat = lambda s: [s[k] for k in ("weight", "exp_avg", "exp_avg_sq")] + \
        [t for k in ("layers", "layers_exp_avg", "layers_exp_avg_sq") for pair in s[k] for t in pair]   # noqa: E731
    return all(torch.equal(x, y) for x, y in zip(flat(sa), flat(sb)))


# ---- the restatement with one fault --------------------------------------------------------------------------------
FAULTS = ("duplicate_dropped", "self_pair_b_dropped", "no_decay_of_untouched_rows", "last_channel_missed",
          "last_tile_partial_dropped", "one_mask_for_both")


def faulty_step(st, pos, neg, masks, p, lr, fault, tile):
    """R.step with one fault a kernel could have; `tile` = pairs per tile of the layout at hand."""
    pos, neg = np.asarray(pos), np.asarray(neg)
    B, n = len(pos), len(st["x"])
    pairs = np.concatenate([pos, neg])
    if fault == "one_mask_for_both":
        masks = np.concatenate([masks[:B], masks[:B]])
    sel = None
    if fault == "last_tile_partial_dropped":
        sel = np.arange(2 * B) < (2 * B - 1) // tile * tile
    _, (ga, gb), glayers, _ = R.loss_and_grads(st["x"], st["layers"], pos, neg, masks, p, True, pred_pairs=sel)
    ga, gb = ga.copy(), gb.copy()
    if fault == "duplicate_dropped":
        seen = {}
        for i, pr in enumerate(map(tuple, pairs)):
            if pr in seen and pr[0] != pr[1]:
                ga[i] = gb[i] = 0
                break
            seen[pr] = i
        else:
            raise AssertionError("no pair is listed twice")
    if fault == "self_pair_b_dropped":
        i = int(np.flatnonzero(pairs[:, 0] == pairs[:, 1])[0])
        gb[i] = 0
    if fault == "last_channel_missed":
        ga[:, -1] = gb[:, -1] = 0
    new = R.apply_grads(st, R.table_grad(n, pairs, ga, gb), glayers, lr)
    if fault == "no_decay_of_untouched_rows":
        idle = np.ones(n, dtype=bool)
        idle[pairs.reshape(-1)] = False
        for k in ("x", "xm", "xv"):
            new[k][idle] = st[k][idle]
    return new
