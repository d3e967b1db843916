"""fp64 restatement of one node2vec training step as PyG 2.0.x `Node2Vec.loss` + `torch.optim.SparseAdam` define it,
written from their contract (PyG is not on this stack): windows -> loss, coalesced sparse gradient, SparseAdam
row update.  numpy only; the host tests check it against torch autograd, the GPU tests check the engine against it.
"""
import numpy as np

EPS = 1e-15
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def windows_of(rw, context_size):
    """PyG pos_sample / neg_sample: walk rows [R, L+1] cut into 1 + L + 1 - C windows of C nodes, concatenated
    window-index-major: torch.cat([rw[:, j:j + C] for j in range(W)], 0)."""
    rw = np.asarray(rw)
    W = rw.shape[1] + 1 - context_size
    return np.concatenate([rw[:, j:j + context_size] for j in range(W)], axis=0)


def loss_and_grad(h, pos, neg, magnitude=False, fp32_sigmoid=False):
    """h [N, D]; pos [P, C], neg [Q, C] windows.  Returns (loss, grad [N, D] dense: the coalesced sparse gradient,
    rows: the sorted unique rows the step touches).  magnitude=True: grad holds Σ|g · h| over the same terms instead
    (the scale of a row's rounding error when its terms are summed in floating point).  fp32_sigmoid=True evaluates
    sigmoid in fp32 as the reference trains: 1 - s is then 0 for every dot past out ~ 16.6, so such a negative
    dot's loss is -log(EPS) and its gradient 0, and near there 1 - s moves in steps of 2^-24."""
    h = np.asarray(h, dtype=np.float64)
    grad = np.zeros_like(h)
    hm = np.abs(h) if magnitude else h
    loss = 0.0
    for win, sign in ((np.asarray(pos), 1), (np.asarray(neg), -1)):
        start, rest = win[:, 0], win[:, 1:]
        out = np.einsum("pd,pcd->pc", h[start], h[rest])            # [P, C-1]
        if fp32_sigmoid:   # the reference's own fp32 evaluation, 1 / (1 + exp(-out)): exactly 1.0 past out ~ 16.6
            with np.errstate(over="ignore"):
                s = (np.float32(1) / (np.float32(1) + np.exp(-out).astype(np.float32))).astype(np.float64)
        else:
            s = 1.0 / (1.0 + np.exp(-out))
        n = out.size
        if sign > 0:
            loss += np.mean(-np.log(s + EPS))
            g = -s * (1.0 - s) / (s + EPS) / n
        else:
            loss += np.mean(-np.log(1.0 - s + EPS))
            g = s * (1.0 - s) / (1.0 - s + EPS) / n
        if magnitude:
            g = np.abs(g)
        np.add.at(grad, start, np.einsum("pc,pcd->pd", g, hm[rest]))
        np.add.at(grad, rest.reshape(-1), (g[:, :, None] * hm[start][:, None, :]).reshape(-1, h.shape[1]))
    rows = np.unique(np.concatenate([np.asarray(pos).reshape(-1), np.asarray(neg).reshape(-1)]))
    return loss, grad, rows


def sparse_adam(h, m, v, step, grad, rows, lr):
    """torch.optim.SparseAdam on the touched rows; `step` is the count AFTER this step (global per parameter)."""
    h, m, v = (np.array(x, dtype=np.float64) for x in (h, m, v))
    g = grad[rows]
    m[rows] = m[rows] + (g - m[rows]) * (1 - BETA1)
    v[rows] = v[rows] + (g * g - v[rows]) * (1 - BETA2)
    step_size = lr * np.sqrt(1 - BETA2 ** step) / (1 - BETA1 ** step)
    h[rows] = h[rows] - step_size * m[rows] / (np.sqrt(v[rows]) + ADAM_EPS)
    return h, m, v


def step(h, m, v, step_count, pos, neg, lr=0.01, fp32_sigmoid=False):
    """One training step from state (h, m, v, step_count): returns (h', m', v', loss)."""
    loss, grad, rows = loss_and_grad(h, pos, neg, fp32_sigmoid=fp32_sigmoid)
    h2, m2, v2 = sparse_adam(h, m, v, step_count + 1, grad, rows, lr)
    return h2, m2, v2, loss
