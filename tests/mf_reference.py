"""The MF baseline restated in fp64 numpy (reference baselines/mf.py read, nothing copied): a table x [N, H], a
predictor of L Linear layers (weight [out, H], bias [out]; out = H but for the last layer's 1) over x[a] ⊙ x[b], relu
and dropout after every hidden layer, sigmoid, the EPS-form losses, dense Adam in torch's operation order.

A state is a dict: x, xm, xv [N, H]; layers, lm, lv: lists of (W, b); t: Adam's step count.  Pairs are [B, 2] arrays,
masks [2B, L-1, H] of 0 / 1 (positives first; None: all kept).  fp32_sigmoid=True rounds the sigmoid to fp32 the way
the engine (and torch on fp32 tensors) evaluates it, which is what makes 1 - s exactly 0 past out ~ 16.6."""
import numpy as np

EPS = 1e-15
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def new_state(x, layers):
    x = np.array(x, dtype=np.float64)
    layers = [(np.array(W, dtype=np.float64), np.array(b, dtype=np.float64)) for W, b in layers]
    return {"x": x, "xm": np.zeros_like(x), "xv": np.zeros_like(x), "layers": layers,
            "lm": [(np.zeros_like(W), np.zeros_like(b)) for W, b in layers],
            "lv": [(np.zeros_like(W), np.zeros_like(b)) for W, b in layers], "t": 0}


def sigmoid(out, fp32=False):
    if not fp32:
        return 1.0 / (1.0 + np.exp(-out))
    with np.errstate(over="ignore"):
        o = out.astype(np.float32)
        return (np.float32(1) / (np.float32(1) + np.exp(-o))).astype(np.float64)


def forward(x, layers, pairs, masks=None, p=0.0, fp32_sigmoid=False):
    """acts [h0, a1, .., a_{L-1}] (the input of every layer), pres (every hidden layer before relu), out [n], s [n].
    masks None and p = 0 is eval mode."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    h = x[pairs[:, 0]] * x[pairs[:, 1]]
    acts, pres = [h], []
    scale = 1.0 / (1.0 - p)
    for l, (W, b) in enumerate(layers[:-1]):
        pre = h @ W.T + b
        h = np.maximum(pre, 0.0)
        if masks is not None:
            h = h * masks[:, l, :] * scale
        pres.append(pre)
        acts.append(h)
    W, b = layers[-1]
    out = (h @ W.T + b)[:, 0]
    return acts, pres, out, sigmoid(out, fp32_sigmoid)


def loss_and_grads(x, layers, pos, neg, masks=None, p=0.0, fp32_sigmoid=False, pred_pairs=None):
    """loss, (ga, gb) [2B, H]: the gradient terms of endpoint a and endpoint b of every pair (positives first),
    glayers [(gW, gb)], and the intermediates (acts, pres, dpres, g).  pred_pairs: a boolean [2B] choice of the pairs
    whose terms enter the predictor's gradients (all of them; a test restating a wrong kernel passes fewer)."""
    pos, neg = np.asarray(pos).reshape(-1, 2), np.asarray(neg).reshape(-1, 2)
    B = len(pos)
    pairs = np.concatenate([pos, neg])
    acts, pres, out, s = forward(x, layers, pairs, masks, p, fp32_sigmoid)
    loss = np.mean(-np.log(s[:B] + EPS)) + np.mean(-np.log(1 - s[B:] + EPS))
    g = np.concatenate([-s[:B] * (1 - s[:B]) / (s[:B] + EPS), s[B:] * (1 - s[B:]) / (1 - s[B:] + EPS)]) / B
    sel = np.ones(2 * B, dtype=bool) if pred_pairs is None else np.asarray(pred_pairs, dtype=bool)
    scale = 1.0 / (1.0 - p)
    d = g[:, None]                                  # d loss / d (output of the layer at hand)
    glayers, dpres = [None] * len(layers), [None] * len(layers)
    for l in range(len(layers) - 1, -1, -1):
        W, _ = layers[l]
        dpres[l] = d
        glayers[l] = (d[sel].T @ acts[l][sel], d[sel].sum(axis=0))
        din = d @ W
        if l > 0:
            keep = np.ones_like(din) if masks is None else masks[:, l - 1, :]
            d = din * (pres[l - 1] > 0) * keep * scale
        else:
            d = din
    ga, gb = d * x[pairs[:, 1]], d * x[pairs[:, 0]]
    return loss, (ga, gb), glayers, {"acts": acts, "pres": pres, "dpres": dpres, "g": g, "out": out, "dh0": d,
                                     "pairs": pairs}


def table_grad(n, pairs, ga, gb):
    """[N, H]: every row's terms added in the step's endpoint-list order (pair-major, endpoint a then b)."""
    gx = np.zeros((n, ga.shape[1]))
    for i, (a, b) in enumerate(pairs):
        gx[a] += ga[i]
        gx[b] += gb[i]
    return gx


def adam(w, m, v, g, t, lr):
    """torch.optim.Adam's update number t (1-based) of one tensor: returns (w', m', v')."""
    m2 = m + (g - m) * (1 - BETA1)
    v2 = v * BETA2 + (1 - BETA2) * g * g
    bc1, bc2 = 1 - BETA1 ** t, 1 - BETA2 ** t
    return w - (lr / bc1) * (m2 / (np.sqrt(v2) / np.sqrt(bc2) + ADAM_EPS)), m2, v2


def apply_grads(st, gx, glayers, lr):
    t = st["t"] + 1
    x, xm, xv = adam(st["x"], st["xm"], st["xv"], gx, t, lr)
    layers, lm, lv = [], [], []
    for (W, b), (mW, mb), (vW, vb), (gW, gb_) in zip(st["layers"], st["lm"], st["lv"], glayers):
        W2, mW2, vW2 = adam(W, mW, vW, gW, t, lr)
        b2, mb2, vb2 = adam(b, mb, vb, gb_, t, lr)
        layers.append((W2, b2))
        lm.append((mW2, mb2))
        lv.append((vW2, vb2))
    return {"x": x, "xm": xm, "xv": xv, "layers": layers, "lm": lm, "lv": lv, "t": t}


def step(st, pos, neg, masks=None, p=0.0, lr=0.01, fp32_sigmoid=False):
    """One dense Adam step: (new state, loss).  Every table row is updated, touched or not."""
    loss, (ga, gb), glayers, aux = loss_and_grads(st["x"], st["layers"], pos, neg, masks, p, fp32_sigmoid)
    return apply_grads(st, table_grad(len(st["x"]), aux["pairs"], ga, gb), glayers, lr), loss


def score(st, pairs, fp32_sigmoid=False):
    pairs = np.asarray(pairs).reshape(-1, 2)
    return forward(st["x"], st["layers"], pairs, None, 0.0, fp32_sigmoid)[3]
