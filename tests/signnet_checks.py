"""What the SIGNNet tests share (tests/test_signnet_host.py, tests/test_gpu_signnet.py, tests/test_gpu_signnet_shapes.py):
row stores, initial values, the shape list of the GPU parity test, and the MEASURED bounds of one teacher-forced step
against the fp64 restatement (tests/signnet_reference.py).

The bound of a gradient tensor is 4 × the largest |fp32 restatement - fp64 restatement| over eight random summation
orders (the kernel's own tree order with FMA contraction is one more draw from that distribution); Adam carries it to
exp_avg, exp_avg_sq and the weights by first-order sensitivity (`mf_checks.adam_bounds`, which also gives every stored
quantity 4 fp32 ulps of its own).  The loss, the running statistics and `score`'s logits get 4 × their own largest
fp32 - fp64 difference plus those 4 ulps.  numpy and torch only; nothing here needs a GPU until a trainer is passed in."""
import numpy as np
import torch

import mf_checks
import signnet_reference as R

ULP = mf_checks.ULP
ORDERS = 8
PARAM_KEYS = ("operator_diff.0.weight", "operator_diff.0.bias", "operator_diff.2.weight", "operator_diff.2.bias",
              "link_pred_mlp.0.weight", "link_pred_mlp.0.bias", "link_pred_mlp.2.weight", "link_pred_mlp.2.bias",
              "link_pred_mlp.4.weight", "link_pred_mlp.4.bias")
STAT_KEYS = {"rm1": "operator_diff.2.running_mean", "rv1": "operator_diff.2.running_var",
             "rm2": "link_pred_mlp.2.running_mean", "rv2": "link_pred_mlp.2.running_var"}
MIN_VARIANCE, RELU_MARGIN = 1e-3, 1e-4      # the conditions on the inputs (asserted from the restatement)

# (H, in_width, B, p, mode, store) of the teacher-forced parity test: H 1, 2, 7, 32, 33, 64, 255, 256; in_width 1, 3,
# 64, 65 (one past the scalar path's tile of 64), 260 (one past the float4 path's tile of 256), 2004; B 2, 3, 32, 33,
# 64; both stores; all three modes; p 0 and 0.5.  They reach all four (k_vector, head_k_vector) layouts.  B = 2 and 3
# go with H = 1 and 2 only: a ReLU column whose B pre-activations are all negative has batch variance 0, which the
# conditions on the inputs exclude, and that happens to one column in 2^B.
SHAPES = [(1, 1, 2, 0.0, "", "two"), (2, 3, 3, 0.5, "mean", "mixed"), (7, 65, 33, 0.5, "sum", "mixed"),
          (32, 64, 32, 0.5, "", "two"), (33, 64, 64, 0.0, "mean", "mixed"), (64, 260, 32, 0.5, "sum", "mixed"),
          (255, 3, 33, 0.5, "", "two"), (256, 2004, 32, 0.5, "mean", "mixed"), (32, 65, 64, 0.5, "", "mixed"),
          (7, 64, 64, 0.5, "mean", "two"), (2, 1, 32, 0.0, "sum", "mixed")]
LAYOUTS = {(1, 1), (1, 4), (4, 1), (4, 4)}      # (k_vector, head_k_vector)
NUM_LINKS = 70
BIG_LINK, BIG_ROWS = 37, 2 + 70                 # one link with more rows than a row tile of 64


# ---- inputs --------------------------------------------------------------------------------------------------------
def make_store(kind, in_width, seed, num_links=NUM_LINKS):
    """(x fp32 [ΣR, in_width] of N(0, 1), row_ptr int64 [L + 1], y fp32 [L]).  "two": every link has its two centre
    rows only; "mixed": 2, 3, 2, 5, .. rows and link BIG_LINK 72; the first and the last link have 2 rows (no
    common-neighbour rows)."""
    rng = np.random.default_rng(seed)
    if kind == "two":
        cnt = np.full(num_links, 2)
    else:
        cnt = np.array([2, 3, 2, 5, 4, 2, 3][:num_links] * (num_links // 7 + 1))[:num_links]
        if num_links > BIG_LINK:
            cnt[BIG_LINK] = BIG_ROWS
        cnt[0] = cnt[-1] = 2
    row_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    x = rng.standard_normal((int(row_ptr[-1]), in_width)).astype(np.float32)
    y = (rng.random(num_links) < 0.5).astype(np.float32)
    return x, row_ptr, y


def batch_ids(B, rng, num_links=NUM_LINKS):
    """B distinct link ids out of order that include the first and the last link of the store and, from 4 on, the big
    link and its neighbour."""
    must = [num_links - 1, 0] + ([BIG_LINK, BIG_LINK + 1] if B >= 4 else [])
    rest = [i for i in rng.permutation(num_links) if i not in must]
    ids = np.array(must + rest[:B - len(must)])
    tail = ids[1:].copy()
    rng.shuffle(tail)
    return np.concatenate([ids[:1], tail]).astype(np.int64)      # the last link comes first


def init_params(H, in_width, ch, seed):
    """fp32 torch-default initial values under the restatement's names."""
    rng = np.random.default_rng(seed)

    def lin(out, fan):
        b = 1 / np.sqrt(fan)
        return rng.uniform(-b, b, (out, fan)).astype(np.float32), rng.uniform(-b, b, out).astype(np.float32)

    W1, b1 = lin(H, in_width)
    W2, b2 = lin(H, ch * H)
    W3, b3 = lin(1, H)
    one, zero = np.ones(H, np.float32), np.zeros(H, np.float32)
    return dict(W1=W1, b1=b1, g1=one, be1=zero, W2=W2, b2=b2, g2=one.copy(), be2=zero.copy(), W3=W3, b3=b3)


def twin_state_dict(params, st=None):
    """The restatement's tensors under SIGNNetTwin's key names, as torch tensors (st: with its running statistics)."""
    sd = {k: torch.as_tensor(np.asarray(params[n], dtype=np.float32)) for k, n in zip(PARAM_KEYS, R.NAMES)}
    H = sd[PARAM_KEYS[1]].numel()
    for n, k in STAT_KEYS.items():
        sd[k] = torch.as_tensor(np.asarray(st[n], np.float32)) if st else (torch.ones(H) if n[:2] == "rv" else torch.zeros(H))
    return sd


def random_masks(R_, B, H, p, rng):
    if not p:
        return None, None
    return (rng.random((R_, H)) >= p).astype(np.uint8), (rng.random((B, H)) >= p).astype(np.uint8)


def state_of(net):
    """The engine's state as a restatement state (fp64 copies)."""
    sd = net.state_dict(optimizer=True)

    def f(t):
        return t.cpu().double().numpy()

    st = {n: f(sd[k]) for k, n in zip(PARAM_KEYS, R.NAMES)}
    st["m"] = {n: f(sd["exp_avg." + k]) for k, n in zip(PARAM_KEYS, R.NAMES)}
    st["v"] = {n: f(sd["exp_avg_sq." + k]) for k, n in zip(PARAM_KEYS, R.NAMES)}
    for n, k in STAT_KEYS.items():
        st[n] = f(sd[k])
    st["t"] = sd["step"]
    st["nbt"] = int(sd["operator_diff.2.num_batches_tracked"])
    assert st["nbt"] == int(sd["link_pred_mlp.2.num_batches_tracked"])
    return st


# ---- bounds --------------------------------------------------------------------------------------------------------
def conditions(f):
    """The conditions on the inputs, from the restatement's forward: (smallest batch variance of a BN column, smallest
    |ReLU pre-activation|)."""
    return float(min(f["var1"].min(), f["var2"].min())), float(np.abs(f["pre2"]).min())


def step_bounds(st, x, row_ptr, y, ids, mask1, mask2, p, mode, lr, seed=0):
    """(the restatement's next state, its loss, bounds, its forward): bounds mirrors the state (the ten names, "m",
    "v", the four running statistics) and has "loss"."""
    new, loss, g64, f = R.step(st, x, row_ptr, y, ids, mask1, mask2, p, mode, lr)
    stats64 = R.running(f, len(ids))
    eg = {k: 0.0 for k in R.NAMES}
    es, el = [0.0] * 4, 0.0
    for o in range(ORDERS):
        S = R.Sums(np.float32, np.random.default_rng([seed, o]))
        l32, g32, f32 = R.loss_and_grads(st, x, row_ptr, y, ids, mask1, mask2, p, mode, S)
        for k in R.NAMES:
            eg[k] = max(eg[k], float(np.max(np.abs(g32[k].astype(np.float64) - g64[k]))))
        for i, (a, b) in enumerate(zip(R.running(f32, len(ids)), stats64)):
            es[i] = max(es[i], float(np.max(np.abs(a.astype(np.float64) - b))))
        el = max(el, abs(float(l32) - loss))
    t = st["t"] + 1
    b = {"m": {}, "v": {}, "loss": 4 * el + ULP * abs(loss)}
    for k in R.NAMES:
        b[k], b["m"][k], b["v"][k] = mf_checks.adam_bounds(st[k], st["m"][k], st["v"][k], g64[k], 4 * eg[k], t, lr)
    for name, e in zip(("rm1", "rv1", "rm2", "rv2"), es):
        b[name] = R.BN_MOMENTUM * 4 * e + ULP * np.abs(new[name])
    return new, loss, b, f


def score_bounds(st, x, row_ptr, mode, seed=0):
    """(the restatement's eval logits, their bound)"""
    ref = R.score(st, x, row_ptr, mode)
    e = 0.0
    for o in range(ORDERS):
        got = R.score(st, x, row_ptr, mode, R.Sums(np.float32, np.random.default_rng([seed, o, 1])))
        e = max(e, float(np.max(np.abs(got.astype(np.float64) - ref))))
    return ref, 4 * e + ULP * np.abs(ref)


def worst_ratio(got, ref, bounds):
    """{name: max |got - ref| / bound} over the ten tensors (w.*), their moments (m.*, v.*) and the running stats."""
    out = {}
    for k in R.NAMES:
        out["w." + k] = float(np.max(np.abs(got[k] - ref[k]) / bounds[k]))
        out["m." + k] = float(np.max(np.abs(got["m"][k] - ref["m"][k]) / bounds["m"][k]))
        out["v." + k] = float(np.max(np.abs(got["v"][k] - ref["v"][k]) / bounds["v"][k]))
    for k in ("rm1", "rv1", "rm2", "rv2"):
        out[k] = float(np.max(np.abs(got[k] - ref[k]) / bounds[k]))
    return out


def step_check(net, store, ids, mask1, mask2, p, mode, worst, tag):
    """One `net.step` against the restatement's step from the same state, inside step_bounds; asserts the conditions
    on the inputs from the restatement; updates worst {name: ratio} in place."""
    x, row_ptr, y = store
    st = state_of(net)
    ref, ref_loss, b, f = step_bounds(st, x, row_ptr, y, ids, mask1, mask2, p, mode, net.lr)
    var, margin = conditions(f)
    assert var >= MIN_VARIANCE and margin >= RELU_MARGIN, f"{tag}: the inputs miss the conditions: {var}, {margin}"
    t = torch.as_tensor
    loss = net.step(t(x), t(row_ptr), t(y), t(ids), None if mask1 is None else t(mask1),
                    None if mask2 is None else t(mask2))
    got = state_of(net)
    assert got["t"] == st["t"] + 1 and got["nbt"] == st["nbt"] + 1
    r = worst_ratio(got, ref, b)
    r["loss"] = abs(loss - ref_loss) / b["loss"]
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{tag}: |engine - restatement| / bound = {bad} (loss {loss!r} vs {ref_loss!r})"
    return loss, ref_loss


def find_seed(H, in_width, B, p, mode, kind, steps=3, lr=1e-3, tries=1000):
    """The first seed whose three restated steps meet the conditions on the inputs (CPU only): the seed of the store,
    the initial values, the batches and the masks of a shape."""
    for seed in range(tries):
        case = Case(H, in_width, B, p, mode, kind, seed, lr)
        st, ok = case.state0(), True
        for ids, m1, m2 in case.batches(steps):
            st, _, _, f = R.step(st, *case.store, ids, m1, m2, p, mode, lr)
            var, margin = conditions(f)
            ok = ok and var >= 2 * MIN_VARIANCE and margin >= 2 * RELU_MARGIN      # room for the engine's own path
        if ok:
            return seed
    raise AssertionError("no seed meets the conditions")


class Case:
    """The inputs of one shape: the store, the initial values and the teacher-forced batches, all from one seed."""

    def __init__(self, H, in_width, B, p, mode, kind, seed, lr=1e-3):
        self.H, self.in_width, self.B, self.p, self.mode, self.kind, self.seed, self.lr = H, in_width, B, p, mode, kind, seed, lr
        self.ch = 2 if mode else 1
        self.store = make_store(kind, in_width, seed)
        self.params = init_params(H, in_width, self.ch, seed + 1000)

    def state0(self):
        return R.new_state(self.params)

    def batches(self, steps=3):
        rng = np.random.default_rng(self.seed + 2000)
        out = []
        for _ in range(steps):
            ids = batch_ids(self.B, rng)
            rows = int((self.store[1][ids + 1] - self.store[1][ids]).sum())
            out.append((ids,) + random_masks(rows, self.B, self.H, self.p, rng))
        return out


# seeds found by find_seed on the CPU (tests/test_signnet_host.py checks that each still meets the conditions)
SEEDS = dict(zip(SHAPES, (1, 1, 2, 3, 11, 0, 714, 8, 2, 0, 1)))
