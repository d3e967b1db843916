"""Test infrastructure: an fp64 pure-torch restatement (any device) of the graph autoencoders of reference
baselines/vgae.py:run_vgae, written from PyG 2.0.x's semantics (GCNConv, GAE / VGAE recon_loss and kl_loss,
edge_index_to_vector's pair keys).  Negatives and reparametrisation noise are passed in.  It checks s3grl_amd.gae;
the product never imports it.

    loss, grads = step(state_dict, x, edge_index, num_nodes, "VGAE", neg, noise)
"""
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
