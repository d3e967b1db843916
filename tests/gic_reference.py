"""Test infrastructure: a pure-torch restatement (any device, any float dtype; fp64 by default) of Graph InfoClust as
the reference runs it (Software/GIC: GICEmbs.py:CalGIC, models/gic.py, layers/cluster.py, layers/discriminator.py,
utils/process.py:normalize_adj): the operator, the Clusterator, both discriminators, the loss and the training loop
with its step-only-when-the-loss-did-not-improve rule.  It checks s3grl_amd.gic; the product never imports it.

    out = forward(sd, x, idx, edge_index, n, beta)          # dict: h1 h2 mu10 Z S logits logits2
    loss, grads, out = step(sd, x, idx, edge_index, n, beta, alpha)
    results, embs, trace = train_loop(edge_index, x, n, lists, dataset, epochs=50, lr=0.01, dim=32, seed=0)

Error bounds.  The engine does the reference's fp32 arithmetic with other summation orders, so its error against the
fp64 truth is a fresh draw from the distribution the reference's own fp32 error comes from.  Every comparison is
therefore held to `bound(ref32, ref64, n)` = 8 x (the reference's fp32-vs-fp64 relative Frobenius error of that very
quantity: from the golden file, or from running this restatement in fp32) + 4·sqrt(n)·2^-24, the probabilistic growth
of one length-n fp32 sum, n = N + d + K, which covers quantities where the reference's fp32 draw happens to be exact
(K = 1: every responsibility is exactly 1).  8 x is the point at which a deviation is to be investigated.
"""
import math

import numpy as np
import torch

U32 = 2.0 ** -24


def rel(a, b):
    """Relative Frobenius error of a against b (fp64)."""
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    den = float(b.norm())
    return float((a - b).norm()) / (den if den > 0 else 1.0)


def floor(n):
    return 4.0 * math.sqrt(n) * U32


def bound(ref32, ref64, n):
    return 8.0 * rel(ref32, ref64) + floor(n)


def hyper_parameters(dataset):
    if dataset in ("cora", "citeseer"):
        return 100, 0.5, 128
    if dataset == "pubmed":
        return 10, 0.75, 32
    return 100, 0.5, 10


# ---- operator ------------------------------------------------------------------------------------------------------
def operator(edge_index, n):
    """normalize_adj(A + I) as COO in fp64, coalesced: (row, col, value) with out = M @ h, M = D·(A + I)ᵀ·D,
    A[src, dst] += 1 per arc, D = rowsum(A + I)^-1/2."""
    ei = torch.as_tensor(np.asarray(edge_index)).long()
    A = torch.zeros((n, n), dtype=torch.float64)
    A.index_put_((ei[0], ei[1]), torch.ones(ei.shape[1], dtype=torch.float64), accumulate=True)
    A = A + torch.eye(n, dtype=torch.float64)
    dinv = A.sum(1).pow(-0.5)
    M = (A * dinv[None, :]).T * dinv[None, :]
    row, col = M.nonzero(as_tuple=True)
    return row, col, M[row, col]


def dense(op, n, dtype=torch.float64):
    row, col, val = op
    M = torch.zeros((n, n), dtype=dtype)
    M.index_put_((torch.as_tensor(row).long(), torch.as_tensor(col).long()), torch.as_tensor(val).to(dtype),
                 accumulate=True)
    return M


# ---- model ---------------------------------------------------------------------------------------------------------
def cluster(data, init, beta, num_iter):
    """layers/cluster.py:cluster."""
    mu = init
    data = data / (data.norm(dim=1)[:, None] + 1e-6)
    for _ in range(num_iter):
        mu = mu / (mu.norm(dim=1)[:, None] + 1e-6)
        dist = data @ mu.T
        r = torch.softmax(beta * dist, dim=1)
        cluster_r = r.sum(dim=0)
        cluster_mean = r.T @ data
        mu = torch.diag(1 / cluster_r) @ cluster_mean
    return mu, torch.softmax(beta * dist, dim=1)


def clusterator(h, init, beta):
    """Clusterator.forward: (Z, S, mu after the 10 detached iterations)."""
    mu10, _ = cluster(h, init, beta, 10)
    mu10 = mu10.clone().detach()
    Z, S = cluster(h, mu10, beta, 1)
    return Z, S, mu10


def cluster_discriminator(S, Z, h1, h2):
    c2 = torch.sigmoid(S @ Z)
    return torch.cat([(h1 * c2).sum(1), (h2 * c2).sum(1)])


def encode(sd, x, M):
    w = sd["gcn.fc.weight"]
    fx = w.T if x is None else x @ w.T
    out = M @ fx + sd["gcn.bias"]
    a = sd["gcn.act.weight"]
    return torch.where(out >= 0, out, a * out)


def forward(sd, x, idx, M, beta):
    """models/gic.py:GIC.forward on the dense operator M; sd: the twin's state_dict in the working dtype."""
    h1 = encode(sd, x, M)
    w = sd["gcn.fc.weight"]
    xs = (torch.eye(M.shape[0], dtype=w.dtype)[idx] if x is None else x[idx])
    h2 = encode(sd, xs, M)
    Z, S, mu10 = clusterator(h1, sd["init"], beta)
    c = torch.sigmoid(h1.mean(0))
    W, b = sd["disc.f_k.weight"][0], sd["disc.f_k.bias"]
    logits = torch.cat([h1 @ (W @ c), h2 @ (W @ c)]) + b
    logits2 = cluster_discriminator(S, Z, h1, h2)
    return {"h1": h1, "h2": h2, "mu10": mu10, "Z": Z, "S": S, "logits": logits[None], "logits2": logits2[None]}


def gic_loss(logits, logits2, alpha):
    n = logits.shape[1] // 2
    lbl = torch.cat([torch.ones(1, n, dtype=logits.dtype), torch.zeros(1, n, dtype=logits.dtype)], 1)
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    return alpha * bce(logits, lbl) + (1 - alpha) * bce(logits2, lbl)


PARAMS = ("gcn.fc.weight", "gcn.bias", "gcn.act.weight", "disc.f_k.weight", "disc.f_k.bias")


def cast(sd, dtype):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in sd.items()}


def step(sd, x, idx, M, beta, alpha, dtype=torch.float64):
    """One teacher-forced forward + backward: (loss, {name: grad}, forward's outputs)."""
    p = {k: (v.detach().to(dtype).clone().requires_grad_(k in PARAMS)) for k, v in sd.items()}
    x = None if x is None else torch.as_tensor(x).to(dtype)
    out = forward(p, x, torch.as_tensor(idx).long(), M.to(dtype), beta)
    loss = gic_loss(out["logits"], out["logits2"], alpha)
    loss.backward()
    return loss.detach(), {k: p[k].grad for k in PARAMS}, {k: v.detach() for k, v in out.items()}


def embed(sd, x, M, beta):
    h1 = encode(sd, x, M)
    Z, S, _ = clusterator(h1, sd["init"], beta)
    return h1, S @ Z, h1.mean(0, keepdim=True), Z


# ---- training loop -------------------------------------------------------------------------------------------------
def xavier(shape, fan_in, fan_out, gen):
    a = math.sqrt(6.0 / (fan_in + fan_out))
    return torch.rand(shape, generator=gen, dtype=torch.float64).mul_(2 * a).sub_(a).float()


def init_state(in_features, dim, K, seed):
    """The twin's initial state_dict, drawn as GICTwin draws it."""
    gen = torch.Generator().manual_seed(int(seed))
    sd = {"gcn.fc.weight": xavier((dim, in_features), in_features, dim, gen), "gcn.bias": torch.zeros(dim),
          "gcn.act.weight": torch.full((1,), 0.25)}
    sd["disc.f_k.weight"] = xavier((1, dim, dim), dim * dim, dim, gen)
    sd["disc.f_k.bias"] = torch.zeros(1)
    sd["init"] = torch.rand((K, dim), generator=gen)
    return sd


def evaluate(embs, lists):
    from s3grl_amd.heuristics import average_precision, roc_auc

    test_pos, test_neg, val_pos, val_neg = [torch.as_tensor(np.asarray(t)).long() for t in lists]
    out = {}
    for name, pos, neg in (("val", val_pos, val_neg), ("test", test_pos, test_neg)):
        pairs = torch.cat([pos, neg], 1)
        s = torch.sigmoid((embs[pairs[0]] * embs[pairs[1]]).sum(1)).numpy()
        y = np.r_[np.ones(pos.shape[1]), np.zeros(neg.shape[1])]
        out[name] = (roc_auc(y, s), average_precision(y, s))
    return {"AUC": (out["val"][0], out["test"][0]), "AP": (out["val"][1], out["test"][1])}


def train_loop(edge_index, x, n, lists, dataset, *, epochs, lr, dim, seed=0, eval_steps=1, step_every_epoch=False,
               permutations=None, state_dict=None, dtype=torch.float64, patience=100):
    """CalGIC's loop in torch on the CPU: (results {'AUC': [(val, test)], 'AP': [...]}, last embs, {'loss': [...],
    'stepped': [...]}).  backward() and step() only on epochs whose loss did NOT improve on the best so far, unless
    step_every_epoch."""
    beta, alpha, K = hyper_parameters(dataset)
    M = dense(operator(edge_index, n), n, dtype)
    sd = state_dict if state_dict is not None else init_state(n if x is None else x.shape[1], dim, K, seed)
    p = {k: torch.as_tensor(v).detach().to(dtype).clone().requires_grad_(k in PARAMS) for k, v in sd.items()}
    x = None if x is None else torch.as_tensor(x).to(dtype)
    opt = torch.optim.Adam([p[k] for k in PARAMS], lr=lr)
    gen = torch.Generator().manual_seed(int(seed) ^ 0x61c)
    results, trace = {"AUC": [], "AP": []}, {"loss": [], "stepped": []}
    best, cnt_wait, embs = 1e9, 0, None
    for epoch in range(epochs):
        opt.zero_grad(set_to_none=True)
        idx = torch.randperm(n, generator=gen) if permutations is None else torch.as_tensor(permutations[epoch]).long()
        out = forward(p, x, idx, M, beta)
        loss = gic_loss(out["logits"], out["logits2"], alpha)
        value = float(loss.detach())
        trace["loss"].append(value)
        improved = value < best
        if improved:
            best, cnt_wait = value, 0
        else:
            cnt_wait += 1
            if cnt_wait == patience:
                break
        if step_every_epoch or not improved:
            loss.backward()
            opt.step()
            trace["stepped"].append(epoch)
        if epoch % eval_steps == 0:
            with torch.no_grad():
                h1 = encode(p, x, M)
                embs = (h1 / h1.norm(dim=1)[:, None]).nan_to_num(nan=0.0)
            res = evaluate(embs, lists)
            for key in results:
                results[key].append(res[key])
    return results, embs, trace


def best_at_first_max(results):
    r = np.asarray(results)
    i = int(np.argmax(r[:, 0]))
    return float(r[i, 0]), float(r[i, 1])


# ---- golden files --------------------------------------------------------------------------------------------------
CASES = ("tiny", "rand300", "usair", "wide", "odd")
OUTPUTS = ("h1", "h2", "mu10", "Z", "S", "logits", "logits2", "loss", "embed_H", "embed_c")


def golden(case):
    """tests/golden/gic_<case>.npz (make_gic_golden.py) as a dict of numpy arrays."""
    from pathlib import Path

    with np.load(Path(__file__).resolve().parent / "golden" / f"gic_{case}.npz") as f:
        return {k: f[k] for k in f.files}


def golden_state(g, dtype=torch.float64):
    return {k[2:]: torch.as_tensor(v).to(dtype) for k, v in g.items() if k.startswith("p_")}


def golden_inputs(g, dtype=torch.float64):
    """(x or None, perm, dense operator from the stored arcs, n, beta, alpha)."""
    n = int(g["num_nodes"])
    x = None if int(g["x_is_eye"]) else torch.as_tensor(g["x"]).to(dtype)
    M = dense(operator(g["arcs"].T, n), n, dtype)
    return x, torch.as_tensor(g["perm"]).long(), M, n, float(g["beta"]), float(g["alpha"])


def stored(g, key, value):
    """`value` cut to the rows the golden file stores of `key` (all of them, except for the large arrays of `wide`)."""
    value = torch.as_tensor(value).detach()
    if key + "_rows" in g:
        value = value.reshape(-1, value.shape[-1])[torch.as_tensor(g[key + "_rows"]).long()]
    return value.reshape(g[key].shape)


def restated(case, dtype=torch.float64):
    """Every output of the golden file from this restatement: {key: tensor} with the file's keys (h1 .. embed_c,
    g_<param>), whole arrays."""
    g = golden(case)
    x, perm, M, n, beta, alpha = golden_inputs(g, dtype)
    sd = golden_state(g, dtype)
    loss, grads, out = step(sd, x, perm, M, beta, alpha, dtype)
    out["loss"] = loss
    out.update({"g_" + k: v for k, v in grads.items()})
    with torch.no_grad():
        _, out["embed_H"], out["embed_c"], _ = embed(sd, x, M, beta)
    return g, out
