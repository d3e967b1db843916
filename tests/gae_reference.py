"""Test infrastructure: an fp64 pure-torch restatement (any device) of the graph autoencoders of reference
baselines/vgae.py:run_vgae, written from PyG 2.0.x's semantics (GCNConv, GAE / VGAE recon_loss and kl_loss,
edge_index_to_vector's pair keys), and of the engine's negative sampling as csrc/s3grl_gae.hip and DESIGN.md §12
document it.  A step takes its negatives and reparametrisation noise as arguments.  It checks s3grl_amd.gae; the
product never imports it.

    loss, grads = step(state_dict, x, edge_index, num_nodes, "VGAE", neg, noise)
    keys = negatives(pos_keys, num_nodes, count, seed, epoch)        # sorted keys; pair_of_key gives the pairs
    grad_z = pair_backward(z, pairs, coef)
"""
import numpy as np
import torch

from seal_nn_reference import gcn_norm, propagate

EPS = 1e-15
MAX_LOGSTD = 10


def pair_key(i, j, n):
    """PyG edge_index_to_vector (no self-loops): i·(N−1) + j − [j > i]."""
    i, j = torch.as_tensor(i).long(), torch.as_tensor(j).long()
    return i * (n - 1) + j - (j > i).long()


def pair_of_key(k, n):
    """vector_to_edge_index: row = k // (N−1), col = k % (N−1), col += [col >= row]."""
    k = torch.as_tensor(k).long()
    i = torch.div(k, n - 1, rounding_mode="floor")
    j = k % (n - 1)
    return i, j + (j >= i).long()


_M32 = np.uint64(0xffffffff)
NEG_TAG = 0x6761655f6e6567   # "gae_neg"


def mix64(x):
    """The splitmix64 finaliser on a numpy uint64 array (arithmetic mod 2^64)."""
    x = np.asarray(x, dtype=np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xbf58476d1ce4e5b9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94d049bb133111eb)
    x ^= x >> np.uint64(31)
    return x


def mulhi64(a, b):
    """floor(a · b / 2^64) for a uint64 array a and a Python integer 0 <= b < 2^64, by 32-bit halves."""
    a = np.asarray(a, dtype=np.uint64)
    b0, b1 = np.uint64(b & 0xffffffff), np.uint64(b >> 32)
    a0, a1 = a & _M32, a >> np.uint64(32)
    mid = a1 * b0 + ((a0 * b0) >> np.uint64(32))          # < 2^64: (2^32−1)^2 + 2^32 − 1
    mid2 = a0 * b1 + (mid & _M32)
    return a1 * b1 + (mid >> np.uint64(32)) + (mid2 >> np.uint64(32))


def negatives(pos_keys, num_nodes, count, seed, epoch, trace=None):
    """The negatives of s3grl_gae_negatives / DESIGN.md §12, the slow way: sorted int64 keys [k], k <= count.

    pos_keys: the keys of the positives that are not self-loops, duplicates included (M = their number, PyG's
    idx.numel()).  pop = N(N−1), prob = 1 − M / pop, S = int(1.1·count / prob) in double arithmetic.  S >= pop
    (compared before truncation): the draws are the keys 0 .. pop−1 in that order.  Else there are 3 rounds of S
    draws; draw i of round r is mulhi(mix(key ^ mix((r << 40) ^ i)), pop) with key = mix(mix(mix(seed mod 2^32) ^
    epoch) ^ NEG_TAG).  The draws are walked in draw order; one is kept when its key is no positive and was not
    drawn before; the walk stops at `count` kept draws.  `trace` (a dict) receives S, T, enumerate and kept_per_round.
    """
    n, count = int(num_nodes), int(count)
    pos = set(np.asarray(pos_keys, dtype=np.int64).tolist())
    M = int(np.asarray(pos_keys).size)
    pop = n * (n - 1)
    info = {"S": 0, "T": 0, "enumerate": False, "kept_per_round": []}
    kept = []
    if M < pop and count > 0:
        prob = 1.0 - M / pop
        s_real = 1.1 * count / prob
        enum = s_real >= pop
        S = pop if enum else int(s_real)
        if enum:
            rounds = [np.arange(pop, dtype=np.uint64)]
        else:
            key = mix64(mix64(mix64(int(seed) & 0xffffffff) ^ np.uint64(int(epoch))) ^ np.uint64(NEG_TAG))
            i = np.arange(S, dtype=np.uint64)
            rounds = [mulhi64(mix64(key ^ mix64(np.uint64(r << 40) ^ i)), pop) for r in range(3)]
        info.update(S=S, T=S * len(rounds), enumerate=bool(enum))
        seen = set()
        for draws in rounds:
            before = len(kept)
            for k in draws.tolist():
                if len(kept) == count:
                    break
                if k in pos or k in seen:
                    continue
                seen.add(k)
                kept.append(k)
            info["kept_per_round"].append(len(kept) - before)
    if trace is not None:
        trace.update(info)
    return torch.tensor(sorted(kept), dtype=torch.int64)


def pair_backward(z, pairs, coef):
    """grad_z of Σ_p coef_p · z_u·z_v over pairs [2, L] (fp64): grad_z[u] += coef·z[v], grad_z[v] += coef·z[u];
    a self pair adds 2·coef·z[u], a duplicated pair adds once per copy."""
    z, coef = z.double(), torch.as_tensor(coef).double()
    pairs = torch.as_tensor(pairs).long()
    g = torch.zeros_like(z)
    g.index_add_(0, pairs[0], coef[:, None] * z[pairs[1]])
    g.index_add_(0, pairs[1], coef[:, None] * z[pairs[0]])
    return g


def conv(sd, prefix, x, src, dst, coef):
    w = sd[prefix + ".lin.weight"].double()
    h = w.T if x is None else x @ w.T
    return propagate(h, src, dst, coef) + sd[prefix + ".bias"].double()


def encode(sd, x, edge_index, num_nodes, model, noise=None):
    """(z, mu, logstd) in fp64; logstd clamped at MAX_LOGSTD; z = mu + noise·exp(logstd) when noise is given (training),
    else mu.  GAE: mu = z, logstd = None."""
    src, dst, coef = gcn_norm(edge_index, num_nodes)
    x = None if x is None else x.double()
    h = torch.relu(conv(sd, "encoder.conv1", x, src, dst, coef))
    if model == "GAE":
        z = conv(sd, "encoder.conv2", h, src, dst, coef)
        return z, z, None
    mu = conv(sd, "encoder.conv_mu", h, src, dst, coef)
    logstd = conv(sd, "encoder.conv_logstd", h, src, dst, coef).clamp(max=MAX_LOGSTD)
    z = mu if noise is None else mu + noise.double() * torch.exp(logstd)
    return z, mu, logstd


def logits(z, pairs):
    pairs = torch.as_tensor(pairs).long()
    return (z[pairs[0]] * z[pairs[1]]).sum(dim=1)


def recon_loss(z, pos, neg):
    pos_loss = -torch.log(torch.sigmoid(logits(z, pos)) + EPS).mean()
    neg_loss = -torch.log(1 - torch.sigmoid(logits(z, neg)) + EPS).mean()
    return pos_loss + neg_loss


def recon_coef(z, pos, neg):
    """d recon_loss / d logit of every pair, positives then negatives (closed form)."""
    s_p, s_n = torch.sigmoid(logits(z, pos)), torch.sigmoid(logits(z, neg))
    P, Q = s_p.numel(), s_n.numel()
    return torch.cat([-(s_p * (1 - s_p)) / (s_p + EPS) / P, (s_n * (1 - s_n)) / (1 - s_n + EPS) / Q])


def kl_loss(mu, logstd):
    return -0.5 * torch.mean(torch.sum(1 + 2 * logstd - mu ** 2 - logstd.exp() ** 2, dim=1))


def training_loss(sd, x, edge_index, num_nodes, model, neg, noise=None, regularise=False):
    """The loss run_vgae backpropagates: recon_loss (+ (1 / max(edge_index)) · kl_loss for VGAE / ARGVA when
    regularise; as written, never)."""
    z, mu, logstd = encode(sd, x, edge_index, num_nodes, model, noise)
    loss = recon_loss(z, edge_index, neg)
    if regularise and model in ("VGAE", "ARGVA"):
        loss = loss + (1 / torch.as_tensor(edge_index).max().double()) * kl_loss(mu, logstd)
    return loss


def step(sd, x, edge_index, num_nodes, model, neg, noise=None, regularise=False):
    """One teacher-forced training step in fp64: (loss, {name: grad}) for every encoder parameter of sd."""
    params = {k: v.detach().double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith("encoder.")}
    loss = training_loss(params, x, edge_index, num_nodes, model, neg, noise, regularise)
    loss.backward()
    return loss.detach(), {k: p.grad for k, p in params.items()}


def best_at_first_max(results):
    """Logger.print_statistics: (val, test) at the first index of the maximal val."""
    r = torch.as_tensor(results)
    i = int(r[:, 0].argmax())
    return float(r[i, 0]), float(r[i, 1])
