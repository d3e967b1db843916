"""Graph autoencoders of the reference's Table 2 and `--init_representation` (baselines/vgae.py:run_vgae,
run_helpers/run_vgae.py, sgrl_link_pred.py:973-1003): twins of PyG GAE, VGAE and ARGVA whose pair work runs as HIP
kernels behind the C ABI (s3grl_gae_*, csrc/s3grl_gae.hip) and whose GCN propagation is s3grl_gcn_propagate over
the whole graph (`GcnGraph`).

    auc, z = run_vgae(edge_index, x, test_and_val, "VGAE", args)      # the reference's call
    results = run_gae(split, "GAE")                                   # {'AUC': (val, test), 'AP': (val, test)}

Same model and training as PyG 2.0.x, as `run_vgae` runs them:
  * encoders: GCNConv = bias-free glorot linear, gcn_norm with add_remaining_self_loops, propagation source ->
    target, then a bias (zeros at init).  GAE: conv1.relu(), conv2.  VGAE / ARGVA: conv1.relu(), then conv_mu and
    conv_logstd, propagated as ONE pass of width 2·emb; logstd clamped at 10; z = mu + randn·exp(logstd) in
    training, mu in eval mode.  x = None is the identity matrix: x @ W is W, no N x N product.
  * recon_loss: -log(sigmoid(z_u·z_v) + 1e-15).mean() over the positives, plus -log(1 - sigmoid + 1e-15).mean()
    over negative_sampling(positives without self-loops + one self-loop per node, N): 2·E + N distinct, uniformly
    random non-edges by PyG's 'sparse' method (3 rounds of int(1.1·count/prob) draws).
  * Adam(lr) on the encoder, one full-graph step per epoch; every eval_steps epochs val / test AUC and AP of
    sigmoid(z_u·z_v) in fp32 in eval mode; the result is the test value at the FIRST epoch of maximal val value.

Quirks of the reference as written are the default: `model` is rebound to the module before its `model == 'ARGVA'`
and `model in ['ARGVA', 'VGAE']` tests, so no model adds the KL term, ARGVA's discriminator is never trained, and
ARGVA trains exactly VGAE's encoder.  `regularise=True` gives the evident intent: + (1 / max(edge_index)) · kl_loss()
(max as written, not max + 1) for VGAE and ARGVA, and 5 steps of the discriminator's own Adam per epoch for ARGVA.
reg_loss is never added in the reference, so even then the discriminator does not touch the encoder.

Parameter init and the reparametrisation noise come from torch generators seeded with `seed`, the negatives from the
engine's counter-based generator keyed by (seed, epoch, round, index): the same distributions as PyG, not its random
streams, so results are not bit-equal to the reference's.  Two runs with one seed are bit-identical.  GPU only; no
CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import _native as N
from .propagate import GcnGraph, _as_pairs, check_ids  # noqa: F401  (this module's API)

MAX_LOGSTD = 10
EPS = 1e-15
MODELS = ("GAE", "VGAE", "ARGVA")


def _engine(device):
    from .engine import default_engine

    return default_engine(device)


def check_device(device):
    """The device the work runs on; RuntimeError for a CPU device or when no HIP device is visible."""
    dev = torch.device(device) if device is not None else None
    if (dev is not None and dev.type == "cpu") or not torch.cuda.is_available():
        raise RuntimeError("graph autoencoders need a HIP device (MI355X); there is no CPU fallback")
    return dev if dev is not None else torch.device("cuda", torch.cuda.current_device())


def _pairs_on(ei, dev):
    ei = ei.to(device=dev, dtype=torch.int32)
    return ei[0].contiguous(), ei[1].contiguous()


# ---- pair structure ------------------------------------------------------------------------------------------------
class PairList:
    """A list of pairs on the device with what the kernels need of it: int32 src / dst, and on demand the sorted keys
    (negative sampling) and the node-major incidence lists (the pair backward)."""

    def __init__(self, edge_index, num_nodes, device=None):
        self.num_nodes = int(num_nodes)
        ei = check_ids(edge_index, self.num_nodes)
        self.engine = _engine(device)
        self.src, self.dst = _pairs_on(ei, self.engine.device)
        self._keys = self._inc = None

    @classmethod
    def _wrap(cls, src, dst, num_nodes, engine):
        p = cls.__new__(cls)
        p.num_nodes, p.engine, p.src, p.dst = int(num_nodes), engine, src, dst
        p._keys = p._inc = None
        return p

    def __len__(self):
        return self.src.numel()

    def keys(self):
        """(sorted uint64 keys as int64 [P], M): M = pairs that are not self-loops (PyG's idx.numel())."""
        if self._keys is None:
            keys = torch.empty(len(self), dtype=torch.int64, device=self.engine.device)
            m = C.c_int64()
            N.check(N.lib().s3grl_gae_keys(self.engine._ctx, self.num_nodes, N.ptr(self.src), N.ptr(self.dst),
                                           len(self), N.ptr(keys), C.byref(m)), "s3grl_gae_keys")
            self._keys = (keys, int(m.value))
        return self._keys

    def incidence(self):
        """(ptr int64 [N+1], slot int32 [2P]): every node's entries 2·pair + side, pairs ascending."""
        if self._inc is None:
            dev = self.engine.device
            ptr = torch.empty(self.num_nodes + 1, dtype=torch.int64, device=dev)
            slot = torch.empty(2 * len(self), dtype=torch.int32, device=dev)
            N.check(N.lib().s3grl_gae_incidence(self.engine._ctx, self.num_nodes, N.ptr(self.src), N.ptr(self.dst),
                                                len(self), N.ptr(ptr), N.ptr(slot)), "s3grl_gae_incidence")
            self._inc = (ptr, slot)
        return self._inc

    def edge_index(self):
        return torch.stack([self.src.long(), self.dst.long()])


def _sample(pos, count, seed, epoch):
    keys, m = pos.keys()
    dev = pos.engine.device
    src = torch.empty(max(count, 0), dtype=torch.int32, device=dev)
    dst = torch.empty(max(count, 0), dtype=torch.int32, device=dev)
    k = C.c_int64()
    N.check(N.lib().s3grl_gae_negatives(pos.engine._ctx, pos.num_nodes, N.ptr(keys), m, int(count),
                                        int(seed) & 0xffffffff, int(epoch), N.ptr(src), N.ptr(dst), C.byref(k)),
            "s3grl_gae_negatives")
    k = int(k.value)
    return PairList._wrap(src[:k], dst[:k], pos.num_nodes, pos.engine)


def negative_sampling(pos, num_nodes, count=None, *, seed, epoch):
    """PyG negative_sampling(pos, num_nodes, count, method='sparse'): int64 [2, k] device tensor of distinct,
    uniformly random ordered non-edges i != j of `pos` (self-loops of `pos` ignored), k = count (default pos.size(1))
    or fewer exactly where PyG returns fewer; in key order (i, then j).  Deterministic per (seed, epoch)."""
    pl = pos if isinstance(pos, PairList) else PairList(pos, num_nodes)
    count = len(pl) if count is None else int(count)
    if count < 0:
        raise ValueError("count must be >= 0")
    return _sample(pl, count, seed, epoch).edge_index()


def recon_negatives(pos, seed, epoch):
    """The negatives PyG recon_loss draws: negative_sampling(pos without self-loops + a self-loop per node, N)."""
    _, m = pos.keys()
    return _sample(pos, m + pos.num_nodes, seed, epoch)


# ---- decoder and loss ----------------------------------------------------------------------------------------------
def _check_z(z, num_nodes):
    if not z.is_cuda:
        raise RuntimeError("the GAE decoder runs on the MI355X only; there is no CPU fallback")
    if z.dtype != torch.float32 or z.dim() != 2 or z.shape[0] != num_nodes:
        raise ValueError(f"z must be float32 [{num_nodes}, D]")
    return z.contiguous()


def _rows(z):
    """z as the kernels read it: contiguous, 16-byte aligned rows (float4 loads)."""
    z = z.contiguous()
    return z if z.data_ptr() % 16 == 0 else z.clone()


def _decode(z, a, b=None, loss=False):
    eng = a.engine
    z = _rows(z)
    P, Q = len(a), len(b) if b is not None else 0
    logits = torch.empty(P + Q, dtype=torch.float32, device=z.device)
    coef = torch.empty(P + Q, dtype=torch.float32, device=z.device) if loss else None
    out = torch.empty(1, dtype=torch.float32, device=z.device) if loss else None
    N.check(N.lib().s3grl_gae_decode(eng._ctx, z.shape[1], N.ptr(z), N.ptr(a.src), N.ptr(a.dst), P,
                                     N.ptr(b.src if b is not None else None), N.ptr(b.dst if b is not None else None),
                                     Q, N.ptr(logits), N.ptr(coef), N.ptr(out)), "s3grl_gae_decode")
    return logits, coef, out


def _pair_backward(z, scale, a, coef_a, b=None, coef_b=None):
    if b is not None and not len(b):
        b = coef_b = None
    if not len(a):                      # the kernel's first list may not be empty: an empty one adds nothing
        if b is None:
            return torch.zeros_like(_rows(z))
        a, coef_a, b, coef_b = b, coef_b, None, None
    pa, sa = a.incidence()
    pb, sb = b.incidence() if b is not None else (None, None)
    z = _rows(z)
    grad = torch.empty_like(z)
    N.check(N.lib().s3grl_gae_backward(a.engine._ctx, a.num_nodes, z.shape[1], N.ptr(z), N.ptr(scale), N.ptr(pa),
                                       N.ptr(sa), N.ptr(a.src), N.ptr(a.dst), N.ptr(coef_a), N.ptr(pb), N.ptr(sb),
                                       N.ptr(b.src if b is not None else None), N.ptr(b.dst if b is not None else None),
                                       N.ptr(coef_b), N.ptr(grad)), "s3grl_gae_backward")
    return grad


class _Decode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, pairs):
        ctx.pairs = pairs
        ctx.save_for_backward(z)
        return _decode(z, pairs)[0]

    @staticmethod
    def backward(ctx, grad_logits):
        (z,) = ctx.saved_tensors
        coef = grad_logits.to(torch.float32).contiguous()
        return _pair_backward(z, None, ctx.pairs, coef), None


class _ReconLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, pos, neg):
        _, coef, loss = _decode(z, pos, neg, loss=True)
        ctx.pos, ctx.neg = pos, neg
        ctx.save_for_backward(z, coef)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad):
        z, coef = ctx.saved_tensors
        P = len(ctx.pos)
        scale = grad.reshape(1).to(torch.float32).contiguous()
        g = _pair_backward(z, scale, ctx.pos, coef[:P], ctx.neg if len(ctx.neg) else None, coef[P:])
        return g, None, None


def inner_product_decode(z, edge_index, sigmoid=False):
    """PyG InnerProductDecoder: z_u·z_v of every pair of edge_index [2, L] (fp32 [L], differentiable in z), or its
    sigmoid."""
    pairs = edge_index if isinstance(edge_index, PairList) else PairList(edge_index, z.shape[0], z.device)
    z = _check_z(z, pairs.num_nodes)
    out = _Decode.apply(z, pairs)
    return torch.sigmoid(out) if sigmoid else out


def recon_loss(z, pos, neg):
    """PyG GAE.recon_loss(z, pos, neg) with the negatives given (`recon_negatives` draws PyG's): a 0-dim fp32 tensor,
    differentiable in z.  pos / neg: PairList or [2, E] edge indices."""
    N_ = z.shape[0]
    pos = pos if isinstance(pos, PairList) else PairList(pos, N_, z.device)
    neg = neg if isinstance(neg, PairList) else PairList(neg, N_, z.device)
    return _ReconLoss.apply(_check_z(z, pos.num_nodes), pos, neg)


# ---- models --------------------------------------------------------------------------------------------------------
class GCNConvParams(nn.Module):
    """GCNConv's parameters: lin.weight [out, in] (glorot), bias [out] (zeros)."""

    def __init__(self, in_channels, out_channels, gen):
        super().__init__()
        a = math.sqrt(6.0 / (in_channels + out_channels))
        self.lin = nn.Linear(in_channels, out_channels, bias=False)
        with torch.no_grad():
            self.lin.weight.copy_(torch.rand((out_channels, in_channels), generator=gen, dtype=torch.float64)
                                  .mul_(2 * a).sub_(a).float())
        self.bias = nn.Parameter(torch.zeros(out_channels))


def _lin(x, weight):
    return weight.t() if x is None else x @ weight.t()   # x = None: identity features, x @ W^T = W^T


class _Encoder(nn.Module):
    pass


class GAETwin(nn.Module):
    """PyG GAE(GCNEncoder(in, out, hidden)): z = conv2(conv1(x).relu())."""
    variational = False

    def __init__(self, in_channels, out_channels, hidden_channels, *, seed=0):
        super().__init__()
        self.in_channels, self.out_channels, self.hidden_channels = int(in_channels), int(out_channels), \
            int(hidden_channels)
        self.seed = int(seed)
        gen = torch.Generator().manual_seed(self.seed)
        self.encoder = _Encoder()
        self.encoder.conv1 = GCNConvParams(self.in_channels, self.hidden_channels, gen)
        self._make_heads(gen)
        self._noise_gen = None

    def _make_heads(self, gen):
        self.encoder.conv2 = GCNConvParams(self.hidden_channels, self.out_channels, gen)

    def _hidden(self, x, graph):
        c = self.encoder.conv1
        return graph.propagate(_lin(x, c.lin.weight), c.bias).relu()

    def encode(self, x, graph, noise=None):
        c = self.encoder.conv2
        return graph.propagate(_lin(self._hidden(x, graph), c.lin.weight), c.bias)

    def decode(self, z, edge_index, sigmoid=True):
        return inner_product_decode(z, edge_index, sigmoid=sigmoid)

    def recon_loss(self, z, pos, neg):
        return recon_loss(z, pos, neg)


class VGAETwin(GAETwin):
    """PyG VGAE(VariationalGCNEncoder(in, out, hidden)): mu and logstd from one propagation of width 2·out."""
    variational = True

    def _make_heads(self, gen):
        self.encoder.conv_mu = GCNConvParams(self.hidden_channels, self.out_channels, gen)
        self.encoder.conv_logstd = GCNConvParams(self.hidden_channels, self.out_channels, gen)

    def randn_like(self, t):
        if self._noise_gen is None or self._noise_gen.device != t.device:
            self._noise_gen = torch.Generator(device=t.device).manual_seed(self.seed ^ 0x5eed)
        return torch.randn(t.shape, generator=self._noise_gen, device=t.device, dtype=t.dtype)

    def encode(self, x, graph, noise=None):
        """z = mu + noise·exp(logstd) in training (noise: given, or drawn), mu in eval mode."""
        e = self.encoder
        w = torch.cat([e.conv_mu.lin.weight, e.conv_logstd.lin.weight], 0)
        b = torch.cat([e.conv_mu.bias, e.conv_logstd.bias], 0)
        out = graph.propagate(_lin(self._hidden(x, graph), w), b)
        mu, logstd = out[:, :self.out_channels], out[:, self.out_channels:]
        self.__mu__, self.__logstd__ = mu, logstd.clamp(max=MAX_LOGSTD)
        if not self.training:
            return mu
        noise = self.randn_like(self.__logstd__) if noise is None else noise
        return mu + noise * torch.exp(self.__logstd__)

    def kl_loss(self, mu=None, logstd=None):
        mu = self.__mu__ if mu is None else mu
        logstd = self.__logstd__ if logstd is None else logstd.clamp(max=MAX_LOGSTD)
        return -0.5 * torch.mean(torch.sum(1 + 2 * logstd - mu ** 2 - logstd.exp() ** 2, dim=1))


class Discriminator(nn.Module):
    """Reference vgae.Discriminator: lin1 relu dropout(0.5) lin2 relu dropout(0.5) lin3, a plain torch MLP (torch's
    default Linear init, drawn from a generator seeded by the twin)."""

    def __init__(self, in_channels, hidden_channels1, hidden_channels2, out_channels, seed=0):
        super().__init__()
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(seed)
            self.lin1 = nn.Linear(in_channels, hidden_channels1)
            self.lin2 = nn.Linear(hidden_channels1, hidden_channels2)
            self.lin3 = nn.Linear(hidden_channels2, out_channels)
        self.seed = int(seed)
        self._gen = None

    def _dropout(self, x):
        if not self.training:
            return x
        if self._gen is None or self._gen.device != x.device:
            self._gen = torch.Generator(device=x.device).manual_seed(self.seed ^ 0xd509)
        keep = torch.rand(x.shape, generator=self._gen, device=x.device) >= 0.5
        return x * keep * 2.0

    def forward(self, x):
        x = self._dropout(torch.relu(self.lin1(x)))
        x = self._dropout(torch.relu(self.lin2(x)))
        return self.lin3(x)


class ARGVATwin(VGAETwin):
    """PyG ARGVA(ARGVAEncoder(in, hidden, out), Discriminator(out, hidden // 4, hidden, out)): VGAE's encoder and a
    discriminator trained by its own loss (see the module docstring for when)."""

    def __init__(self, in_channels, out_channels, hidden_channels, *, seed=0):
        super().__init__(in_channels, out_channels, hidden_channels, seed=seed)
        self.discriminator = Discriminator(out_channels, hidden_channels // 4, hidden_channels, out_channels,
                                           seed=seed + 1)

    def reg_loss(self, z):
        real = torch.sigmoid(self.discriminator(z))
        return -torch.log(real + EPS).mean()

    def discriminator_loss(self, z):
        real = torch.sigmoid(self.discriminator(self.randn_like(z)))
        fake = torch.sigmoid(self.discriminator(z.detach()))
        return -torch.log(real + EPS).mean() + -torch.log(1 - fake + EPS).mean()


TWINS = {"GAE": GAETwin, "VGAE": VGAETwin, "ARGVA": ARGVATwin}


# ---- training ------------------------------------------------------------------------------------------------------
def best_at_first_max(results):
    """utils.Logger.print_statistics' choice: (val, test) at the FIRST index of the maximal val value."""
    r = np.asarray(results)
    i = int(np.argmax(r[:, 0]))
    return r[i, 0], r[i, 1]


def _scores(z, pairs):
    return torch.sigmoid(_decode(z, pairs)[0]).cpu().numpy()


def _evaluate(z, lists):
    from .heuristics import average_precision, roc_auc

    out = {}
    for name, (pos, neg) in lists.items():
        s = _scores(z, PairList._wrap(torch.cat([pos.src, neg.src]), torch.cat([pos.dst, neg.dst]), pos.num_nodes,
                                      pos.engine))
        y = np.r_[np.ones(len(pos)), np.zeros(len(neg))]
        out[name] = (roc_auc(y, s), average_precision(y, s))
    return {"AUC": (out["val"][0], out["test"][0]), "AP": (out["val"][1], out["test"][1])}


def train(edge_index, x, test_and_val, model, *, epochs=50, hidden=64, emb=32, lr=0.01, eval_steps=1, seed=0,
          regularise=False, num_nodes=None, device=None, log_file=None, on_epoch=None):
    """The loop of run_vgae: returns (per-eval results {'AUC': [(val, test)], 'AP': [...]}, z of the last
    evaluation as fp32 device tensor, per-epoch losses as fp32 device tensor)."""
    if model not in MODELS:
        raise NotImplementedError(f"Model f{model} is not supported.")
    ei = _as_pairs(edge_index)
    if x is not None:
        x = torch.as_tensor(x)
        if x.dim() != 2:
            raise ValueError("x must be [N, F]")
        n = x.shape[0] if num_nodes is None else int(num_nodes)
        if x.shape[0] != n:
            raise ValueError(f"x has {x.shape[0]} rows, the graph {n} nodes")
    else:
        if num_nodes is None:
            raise ValueError("x = None (identity features) needs num_nodes")
        n = int(num_nodes)
    lists = [check_ids(t, n) for t in test_and_val]
    check_ids(ei, n)
    epochs, eval_steps = int(epochs), int(eval_steps)
    if epochs < 0 or eval_steps < 1 or not lr > 0:
        raise ValueError("need epochs >= 0, eval_steps >= 1 and lr > 0")
    dev = check_device(device)

    eng = _engine(dev)
    dev = eng.device
    xs = x.to(device=dev, dtype=torch.float32).contiguous() if x is not None else None
    in_channels = n if x is None else x.shape[1]
    net = TWINS[model](in_channels, emb, hidden, seed=seed).to(dev)
    opt = torch.optim.Adam(net.encoder.parameters(), lr=lr)
    disc_opt = torch.optim.Adam(net.discriminator.parameters(), lr=lr) if model == "ARGVA" else None
    graph = GcnGraph(ei, n, dev)
    pos = PairList(ei, n, dev)
    pos.keys()
    pos.incidence()
    test_pos, test_neg, val_pos, val_neg = (PairList(t, n, dev) for t in lists)
    eval_lists = {"val": (val_pos, val_neg), "test": (test_pos, test_neg)}
    num_nodes_max = torch.max(ei.to(dev)) if ei.numel() else None
    results = {"AUC": [], "AP": []}
    losses = torch.empty(epochs, dtype=torch.float32, device=dev)
    z_last = None
    for epoch in range(1, epochs + 1):
        net.train()
        opt.zero_grad(set_to_none=True)
        z = net.encode(xs, graph)
        if regularise and model == "ARGVA":
            for _ in range(5):
                disc_opt.zero_grad(set_to_none=True)
                net.discriminator_loss(z).backward()
                disc_opt.step()
        neg = recon_negatives(pos, seed, epoch)
        loss = net.recon_loss(z, pos, neg)
        if regularise and net.variational:
            loss = loss + (1 / num_nodes_max) * net.kl_loss()
        loss.backward()
        opt.step()
        losses[epoch - 1] = loss.detach()
        if on_epoch is not None:
            on_epoch(epoch)
        if epoch % eval_steps == 0:
            net.eval()
            with torch.no_grad():
                z_last = net.encode(xs, graph).detach().clone()
            res = _evaluate(z_last, eval_lists)
            for key in results:
                results[key].append(res[key])
            if log_file is not None:
                with open(log_file, "a") as f:
                    for key, (v, t) in res.items():
                        print(f"{key}\nRun: 01, Epoch: {epoch:02d}, Loss: {float(loss):.4f}, Valid: {100 * v:.2f}%, "
                              f"Test: {100 * t:.2f}%", file=f)
    return results, z_last, losses


def run_vgae(edge_index, x, test_and_val, model, args, *, regularise=False, seed=0, device=None, log_file=None):
    """Reference baselines/vgae.run_vgae: trains `model` ('GAE', 'VGAE' or 'ARGVA'; anything else raises
    NotImplementedError) on edge_index [2, E] with features x [N, F] for args.epochs epochs (args.embedding_dim,
    args.hidden_channels, args.lr, args.eval_steps), evaluating on test_and_val = [test_pos, test_neg, val_pos,
    val_neg] ([2, L] each).  Returns (test AUC · 100 at the first epoch of maximal val AUC, as a float; z of the last
    evaluation, a detached fp32 CPU tensor [N, embedding_dim]).  x = None stands for eye(N), N = max id + 1 of all
    lists.  `log_file` (optional) receives the reference's per-eval lines; nothing is written by default."""
    if model not in MODELS:
        raise NotImplementedError(f"Model f{model} is not supported.")
    num_nodes = None
    if x is None:
        num_nodes = 1 + max(int(_as_pairs(t).max()) for t in [edge_index] + list(test_and_val) if _as_pairs(t).numel())
    results, z, _ = train(edge_index, x, test_and_val, model, epochs=args.epochs, hidden=args.hidden_channels,
                          emb=int(args.embedding_dim), lr=args.lr, eval_steps=getattr(args, "eval_steps", 1),
                          seed=seed, regularise=regularise, num_nodes=num_nodes, device=device, log_file=log_file)
    if not results["AUC"]:
        raise ValueError("no evaluation ran: args.epochs < args.eval_steps")
    r = (100 * torch.tensor(results["AUC"])).numpy()   # fp32, as Logger.print_statistics
    return float(best_at_first_max(r)[1]), z.cpu().clone().detach()


def _split_lists(split):
    return [split.links["test"][0], split.links["test"][1], split.links["valid"][0], split.links["valid"][1]]


def run_gae(split, model, x=None, *, epochs=50, hidden=64, emb=32, lr=0.01, seed=1, regularise=False, device=None):
    """One Table 2 autoencoder row from a `workloads.Split` (run_helpers/run_vgae.py: 50 epochs, hidden 64, embedding
    32, lr 0.01, eval every epoch; x = None is eye(N)): {'AUC': (best val, test at it), 'AP': (...)}, each chosen at
    the first epoch of its own maximal val value, as fractions (like heuristics.run_heuristic)."""
    results, _, _ = train(split.edge_index(), x, _split_lists(split), model, epochs=epochs, hidden=hidden, emb=emb,
                          lr=lr, eval_steps=1, seed=seed, regularise=regularise, num_nodes=split.num_nodes,
                          device=device)
    if not results["AUC"]:
        raise ValueError("epochs must be >= 1")
    return {k: tuple(float(v) for v in best_at_first_max(r)) for k, r in results.items()}


def reference_args(epochs=50, embedding_dim=32, hidden_channels=64, lr=0.01, eval_steps=1, log_steps=1):
    """The run helper's DummyArgs fields run_vgae reads."""
    return SimpleNamespace(epochs=epochs, embedding_dim=embedding_dim, hidden_channels=hidden_channels, lr=lr,
                           eval_steps=eval_steps, log_steps=log_steps, res_dir="")
