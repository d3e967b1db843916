"""Graph InfoClust, the fourth `--init_representation` of the reference and the GIC row of its Table 2
(Software/GIC/GICEmbs.py:CalGIC, baselines/run_helpers/run_gic.py, sgrl_link_pred.py:989-996): a twin of models/gic.py
whose soft k-means "Clusterator" and cluster discriminator run as HIP kernels behind the C ABI (s3grl_gic_*,
csrc/s3grl_gic.hip) and whose propagation is s3grl_gcn_propagate over `GicGraph`.

    auc, embs = CalGIC(edge_index, features, dataset, test_and_val, args)     # the reference's call
    results = run_gic(split, "usair")                                         # {'AUC': (val, test), 'AP': (val, test)}

Same model and training as the reference:
  * encoder: h = PReLU(D·(A + I)ᵀ·D · fc(x) + bias), fc a bias-free xavier linear.  The corrupted branch is the same
    encoder on x[idx], idx a fresh node permutation per epoch; since fc(x[idx]) = fc(x)[idx], both branches come from
    ONE linear and ONE propagation of width 2·d.  features = None is the identity matrix: fc(eye) = Wᵀ.
  * Clusterator: 10 detached soft k-means iterations from the fixed, never trained `init`, then 1 differentiable one
    (mu is detached between them): Z [K, d], S [N, K].
  * logits  = bilinear discriminator of h1 / h2 against the summary c = sigmoid(mean(h1)): h @ (W c) + b;
    logits2 = h1[n] · c2[n] and h2[n] · c2[n] with c2 = sigmoid(S @ Z);
    loss = alpha · BCE(logits, [1 | 0]) + (1 - alpha) · BCE(logits2, [1 | 0]).
  * Adam(lr), no weight decay, patience 100; every eval_steps epochs (epochs count from 0) embs = h1 / ‖h1‖ with nan ->
    0 and val / test AUC and AP of sigmoid(embs_u · embs_v) over the given pair lists; the result is the test value
    at the FIRST epoch of maximal val value; the returned embs are those of the LAST evaluated epoch.

Quirk of the reference as written, and the default here: `loss.backward()` and `optimiser.step()` sit in the `else`
branch of `if loss < best` (GICEmbs.py:156-166), so a step is taken ONLY on epochs whose loss did not improve on the
best so far, and epoch 0 never steps.  `step_every_epoch=True` gives the evident intent: a step on every epoch.

Parameter init, `init` and the per-epoch permutation come from torch generators seeded with `args.seed`: the same
distributions as the reference, not its random streams, so results are not bit-equal to the reference's.  Two runs
with one seed are bit-identical.  GPU only; no CPU fallback.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _native as N
from .propagate import GicGraph, _as_pairs, check_ids

CHUNK = 64            # kGicChunk of csrc/s3grl_gic.hip: nodes per workgroup and per partial sum
TILE = 64             # kGicTile: the K tile and d tile of its products
PATIENCE = 100
DETACHED_ITERS = 10


def hyper_parameters(dataset):
    """(beta, alpha, num_clusters) of GICEmbs.py:94-108."""
    if dataset in ("cora", "citeseer"):
        return 100, 0.5, 128
    if dataset == "pubmed":
        return 10, 0.75, 32
    return 100, 0.5, 10


def check_device(device):
    """The device the work runs on; RuntimeError for a CPU device or when no HIP device is visible."""
    dev = torch.device(device) if device is not None else None
    if (dev is not None and dev.type == "cpu") or not torch.cuda.is_available():
        raise RuntimeError("Graph InfoClust needs a HIP device (MI355X); there is no CPU fallback")
    return dev if dev is not None else torch.device("cuda", torch.cuda.current_device())


def check_shape(num_nodes, dim, num_clusters):
    """ValueError unless the kernels take N nodes, d channels and K clusters."""
    if not 1 <= num_nodes < 2**31:
        raise ValueError(f"GIC kernels need 1 <= N < 2^31 nodes, got {num_nodes}")
    if not 1 <= dim <= N.GIC_MAX_DIM:
        raise ValueError(f"GIC kernels need 1 <= d <= {N.GIC_MAX_DIM} channels, got {dim}")
    if not 1 <= num_clusters <= N.GIC_MAX_CLUSTERS:
        raise ValueError(f"GIC kernels need 1 <= K <= {N.GIC_MAX_CLUSTERS} clusters, got {num_clusters}")


def _engine(device):
    from .engine import default_engine

    return default_engine(device)


def _rows(t):
    """(t, row stride) as the kernels read a matrix: unit column stride; a column slice stays a view, anything else
    is copied."""
    if t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        t = t.contiguous()
    return t, t.stride(0)


def _check(t, shape, what):
    if not t.is_cuda:
        raise RuntimeError("the GIC kernels run on the MI355X only; there is no CPU fallback")
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be float32 {list(shape)}, got {t.dtype} {list(t.shape)}")


# ---- soft k-means --------------------------------------------------------------------------------------------------
def _normalise(h):
    h, ld = _rows(h)
    n, d = h.shape
    data = torch.empty((n, d), dtype=torch.float32, device=h.device)
    nrm = torch.empty(n, dtype=torch.float32, device=h.device)
    N.check(N.lib().s3grl_gic_normalise(_engine(h.device)._ctx, n, d, N.ptr(h), ld, N.ptr(data), N.ptr(nrm)),
            "s3grl_gic_normalise")
    return data, nrm


def _cluster(data, init, beta, num_iter):
    """(mu, r, cluster_r, mun) of num_iter iterations on normalised data; nothing is differentiable."""
    n, d = data.shape
    K = init.shape[0]
    dev = data.device
    init = init.contiguous()
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
    mu, r, cr, mun = new(K, d), new(n, K), new(K), new(K, d)
    tmp = new(K, d) if num_iter > 1 else None
    partial = new(-(-n // CHUNK) * (K + K * d))
    N.check(N.lib().s3grl_gic_cluster_forward(_engine(dev)._ctx, n, d, K, float(beta), int(num_iter), N.ptr(data),
                                              N.ptr(init), N.ptr(mun), N.ptr(tmp), N.ptr(partial), N.ptr(mu),
                                              N.ptr(cr), N.ptr(r)), "s3grl_gic_cluster_forward")
    return mu, r, cr, mun


class _Clusterator(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, init, beta, detached_iters):
        data, nrm = _normalise(h)
        mu0 = _cluster(data, init, beta, detached_iters)[0] if detached_iters else init
        Z, S, cr, mun = _cluster(data, mu0, beta, 1)
        ctx.beta = beta
        ctx.save_for_backward(h, data, nrm, mun, S, Z, cr)
        return Z, S

    @staticmethod
    def backward(ctx, gZ, gS):
        h, data, nrm, mun, S, Z, cr = ctx.saved_tensors
        n, d = data.shape
        K = Z.shape[0]
        gZ = torch.zeros_like(Z) if gZ is None else gZ.contiguous()
        gS = torch.zeros_like(S) if gS is None else gS.contiguous()
        h, ld = _rows(h)
        ws = torch.empty(K * d + K, dtype=torch.float32, device=h.device)
        g_h = torch.empty((n, d), dtype=torch.float32, device=h.device)
        N.check(N.lib().s3grl_gic_cluster_backward(_engine(h.device)._ctx, n, d, K, float(ctx.beta), N.ptr(data),
                                                   N.ptr(h), ld, N.ptr(nrm), N.ptr(mun), N.ptr(S), N.ptr(Z), N.ptr(cr),
                                                   N.ptr(gZ), N.ptr(gS), N.ptr(ws), N.ptr(g_h)),
                "s3grl_gic_cluster_backward")
        return g_h, None, None, None


def cluster(h, init, beta, num_iter):
    """Reference layers/cluster.py:cluster(h, K, 1, num_iter, init, beta) on h [N, d] fp32: (mu [K, d], r [N, K]) after
    num_iter >= 1 iterations, r from the last iteration's incoming mu.  Detached."""
    if h.dim() != 2 or init.dim() != 2:
        raise ValueError("h must be [N, d] and init [K, d]")
    _check(h, (h.shape[0], init.shape[1]), "h")
    _check(init, init.shape, "init")
    check_shape(h.shape[0], h.shape[1], init.shape[0])
    if num_iter < 1:
        raise ValueError("num_iter must be >= 1")
    mu, r, _, _ = _cluster(_normalise(h.detach())[0], init.detach(), beta, num_iter)
    return mu, r


def clusterator(h, init, beta, detached_iters=DETACHED_ITERS):
    """Reference Clusterator.forward(h, beta): `detached_iters` detached iterations from `init`, then one iteration
    from that result.  (Z [K, d], S [N, K]), differentiable in h through the last iteration only."""
    if h.dim() != 2 or init.dim() != 2:
        raise ValueError("h must be [N, d] and init [K, d]")
    _check(h, (h.shape[0], init.shape[1]), "h")
    _check(init, init.shape, "init")
    check_shape(h.shape[0], h.shape[1], init.shape[0])
    return _Clusterator.apply(h, init.detach(), float(beta), int(detached_iters))


# ---- cluster discriminator -----------------------------------------------------------------------------------------
def _pair_rows(h1, h2):
    h1, l1 = _rows(h1)
    h2, l2 = _rows(h2)
    if l1 != l2:
        h1, h2 = h1.contiguous(), h2.contiguous()
        l1 = h1.stride(0)
    return h1, h2, l1


class _ClusterDisc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, Z, h1, h2):
        S, Z = S.contiguous(), Z.contiguous()
        h1, h2, ld = _pair_rows(h1, h2)
        n, d = h1.shape
        K = Z.shape[0]
        logits = torch.empty(2 * n, dtype=torch.float32, device=S.device)
        N.check(N.lib().s3grl_gic_disc_forward(_engine(S.device)._ctx, n, d, K, N.ptr(S), N.ptr(Z), N.ptr(h1),
                                               N.ptr(h2), ld, N.ptr(logits)), "s3grl_gic_disc_forward")
        ctx.save_for_backward(S, Z, h1, h2)
        return logits

    @staticmethod
    def backward(ctx, grad):
        S, Z, h1, h2 = ctx.saved_tensors
        h1, h2, ld = _pair_rows(h1, h2)
        n, d = h1.shape
        K = Z.shape[0]
        dev = S.device
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        grad = grad.to(torch.float32).contiguous()
        g_h = new(n, 2 * d)
        gS, gZ, g_pre, partial = new(n, K), new(K, d), new(n, d), new(-(-n // CHUNK) * K * d)
        N.check(N.lib().s3grl_gic_disc_backward(_engine(dev)._ctx, n, d, K, N.ptr(S), N.ptr(Z), N.ptr(h1), N.ptr(h2),
                                                ld, N.ptr(grad), N.ptr(g_h), N.ptr(g_h[:, d:]), 2 * d, N.ptr(g_pre),
                                                N.ptr(partial), N.ptr(gS), N.ptr(gZ)), "s3grl_gic_disc_backward")
        return gS, gZ, g_h[:, :d], g_h[:, d:]


def cluster_discriminator(S, Z, h1, h2):
    """Reference Discriminator_cluster on c2 = sigmoid(S @ Z): fp32 [2N], h1[n] · c2[n] then h2[n] · c2[n]; c2 is never
    formed in memory.  Differentiable in all four."""
    if S.dim() != 2 or Z.dim() != 2:
        raise ValueError("S must be [N, K] and Z [K, d]")
    n, K, d = S.shape[0], Z.shape[0], Z.shape[1]
    _check(S, (n, K), "S")
    _check(Z, (K, d), "Z")
    _check(h1, (n, d), "h1")
    _check(h2, (n, d), "h2")
    check_shape(n, d, K)
    return _ClusterDisc.apply(S, Z, h1, h2)


# ---- model ---------------------------------------------------------------------------------------------------------
def _xavier(shape, fan_in, fan_out, gen):
    a = math.sqrt(6.0 / (fan_in + fan_out))
    return torch.rand(shape, generator=gen, dtype=torch.float64).mul_(2 * a).sub_(a).float()


class _GCN(nn.Module):
    def __init__(self, in_features, hidden, gen):
        super().__init__()
        self.fc = nn.Linear(in_features, hidden, bias=False)
        with torch.no_grad():
            self.fc.weight.copy_(_xavier((hidden, in_features), in_features, hidden, gen))
        self.bias = nn.Parameter(torch.zeros(hidden))
        self.act = nn.PReLU()


class _Bilinear(nn.Module):
    def __init__(self, hidden, gen):
        super().__init__()
        self.f_k = nn.Bilinear(hidden, hidden, 1)
        with torch.no_grad():   # xavier on [1, d, d]: fan_in = d·d, fan_out = d
            self.f_k.weight.copy_(_xavier((1, hidden, hidden), hidden * hidden, hidden, gen))
            self.f_k.bias.zero_()


class GICTwin(nn.Module):
    """Reference models/gic.py:GIC(num_nodes, in_features, hidden, 'prelu', num_clusters, beta), with the reference's
    parameter names (gcn.fc.weight, gcn.bias, gcn.act.weight, disc.f_k.weight, disc.f_k.bias) and `init`, the
    Clusterator's fixed start rand(K, hidden), as a buffer."""

    def __init__(self, num_nodes, in_features, hidden, num_clusters, beta, seed=0):
        super().__init__()
        check_shape(int(num_nodes), int(hidden), int(num_clusters))
        self.num_nodes, self.hidden, self.num_clusters, self.beta = int(num_nodes), int(hidden), int(num_clusters), beta
        gen = torch.Generator().manual_seed(int(seed))
        self.gcn = _GCN(int(in_features), self.hidden, gen)
        self.disc = _Bilinear(self.hidden, gen)
        self.register_buffer("init", torch.rand((self.num_clusters, self.hidden), generator=gen))
        self._ptr = None

    def _lin(self, x):
        w = self.gcn.fc.weight
        return w.t() if x is None else x @ w.t()         # x = None: identity features

    def _readout(self, h1):
        from .mpnn import segment_mean

        if self._ptr is None or self._ptr.device != h1.device:
            self._ptr = torch.tensor([0, self.num_nodes], dtype=torch.int64, device=h1.device)
        return segment_mean(h1, self._ptr, self.num_nodes)            # [1, d], a fixed summation order

    def encode(self, x, graph):
        """h1 [N, d] = PReLU(graph · fc(x) + bias)."""
        return self.gcn.act(graph.propagate(self._lin(x).contiguous(), self.gcn.bias))

    def forward(self, x, idx, graph, beta=None):
        """(logits [1, 2N], logits2 [1, 2N]) of features x (None: eye) and their row permutation idx; beta: this
        call's cluster temperature (default: the model's; the model's is not changed)."""
        beta = self.beta if beta is None else beta
        d = self.hidden
        fx = self._lin(x)
        both = graph.propagate(torch.cat([fx, fx[idx]], 1), torch.cat([self.gcn.bias, self.gcn.bias]))
        hh = self.gcn.act(both)
        h1, h2 = hh[:, :d], hh[:, d:]
        Z, S = clusterator(h1, self.init, beta)
        c = torch.sigmoid(self._readout(h1))[0]
        v = self.disc.f_k.weight[0] @ c                              # f_k(h, c) = h · (W c) + b
        logits = torch.cat([h1 @ v, h2 @ v]) + self.disc.f_k.bias
        logits2 = cluster_discriminator(S, Z, h1, h2)
        return logits[None], logits2[None]

    def embed(self, x, graph):
        """(h1, S @ Z, c, Z), detached; c = mean(h1) without the sigmoid, as in the reference."""
        with torch.no_grad():
            h1 = self.encode(x, graph)
            Z, S = clusterator(h1, self.init, self.beta)
            return h1, S @ Z, self._readout(h1), Z


def gic_loss(logits, logits2, alpha):
    n = logits.shape[1] // 2
    lbl = torch.cat([torch.ones(1, n, device=logits.device), torch.zeros(1, n, device=logits.device)], 1)
    return alpha * F.binary_cross_entropy_with_logits(logits, lbl) + \
        (1 - alpha) * F.binary_cross_entropy_with_logits(logits2, lbl)


# ---- training ------------------------------------------------------------------------------------------------------
def train(edge_index, features, dataset, test_and_val, *, epochs, lr, embedding_dim, eval_steps=1, seed=0,
          num_nodes=None, step_every_epoch=False, permutations=None, state_dict=None, device=None, trace=None):
    """The loop of CalGIC: (per-eval results {'AUC': [(val, test)], 'AP': [...]}, embs of the last evaluation as an
    fp32 device tensor).  permutations: [epochs, N] node permutations instead of the generator's; state_dict: initial
    parameters (and `init`); trace: a dict that receives 'loss' (per epoch), 'stepped' (the epochs that stepped) and
    'hyper_parameters' (beta, alpha, K)."""
    from .gae import PairList, _evaluate

    ei = _as_pairs(edge_index)
    if features is not None:
        features = torch.as_tensor(features)
        if features.dim() != 2:
            raise ValueError("features must be [N, F]")
        n = features.shape[0]
    else:
        if num_nodes is None:
            raise ValueError("features = None (identity features) needs num_nodes")
        n = int(num_nodes)
    lists = [check_ids(t, n) for t in test_and_val]
    check_ids(ei, n)
    epochs, eval_steps = int(epochs), int(eval_steps)
    if epochs < 0 or eval_steps < 1 or not lr > 0:
        raise ValueError("need epochs >= 0, eval_steps >= 1 and lr > 0")
    beta, alpha, K = hyper_parameters(dataset)
    check_shape(n, int(embedding_dim), K)
    dev = _engine(check_device(device)).device

    x = features.to(device=dev, dtype=torch.float32).contiguous() if features is not None else None
    net = GICTwin(n, n if x is None else x.shape[1], int(embedding_dim), K, beta, seed=seed)
    if state_dict is not None:
        net.load_state_dict(state_dict)
    net = net.to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=lr, weight_decay=0.0)
    graph = GicGraph(ei, n, dev)
    test_pos, test_neg, val_pos, val_neg = (PairList(t, n, dev) for t in lists)
    eval_lists = {"val": (val_pos, val_neg), "test": (test_pos, test_neg)}
    gen = torch.Generator().manual_seed(int(seed) ^ 0x61c)
    results = {"AUC": [], "AP": []}
    losses, stepped = [], []
    embs = None
    best, cnt_wait = 1e9, 0
    for epoch in range(epochs):
        net.train()
        opt.zero_grad(set_to_none=True)
        idx = torch.randperm(n, generator=gen) if permutations is None else torch.as_tensor(permutations[epoch])
        logits, logits2 = net(x, idx.to(dev), graph, beta)
        loss = gic_loss(logits, logits2, alpha)
        value = float(loss.detach())
        losses.append(value)
        improved = value < best
        if improved:
            best, cnt_wait = value, 0
        else:
            cnt_wait += 1
            if cnt_wait == PATIENCE:
                break
        if step_every_epoch or not improved:
            loss.backward()
            opt.step()
            stepped.append(epoch)
        if epoch % eval_steps == 0:
            net.eval()
            with torch.no_grad():
                h1 = net.encode(x, graph)
                embs = (h1 / h1.norm(dim=1)[:, None]).nan_to_num(nan=0.0).contiguous()
            res = _evaluate(embs, eval_lists)
            for key in results:
                results[key].append(res[key])
    if trace is not None:
        trace.update(loss=losses, stepped=stepped, hyper_parameters=(beta, alpha, K))
    return results, embs


def CalGIC(edge_index, features, dataset, test_and_val, args, *, step_every_epoch=False, permutations=None,
           state_dict=None, num_nodes=None, device=None, trace=None):
    """Reference GICEmbs.py:CalGIC: trains Graph InfoClust on edge_index [2, E] with features [N, F] (None: eye(N),
    N = num_nodes) for args.epochs epochs (args.lr, args.embedding_dim, args.eval_steps, args.seed), evaluating on
    test_and_val = [test_pos, test_neg, val_pos, val_neg] ([2, L] each).  Returns (test AUC ·
    100 at the first evaluation of maximal val AUC, as a float; the row-normalised embeddings of the LAST evaluation, a
    detached fp32 CPU tensor [N, embedding_dim]).  As in the reference, beta, alpha and the number of clusters follow
    `args.data_name` (GICEmbs.py:97-108), not the positional `dataset`, which there only names a checkpoint file;
    `dataset` is used when args has no data_name."""
    from .gae import best_at_first_max

    check_device(device)
    results, embs = train(edge_index, features, getattr(args, "data_name", dataset), test_and_val,
                          epochs=args.epochs, lr=args.lr,
                          embedding_dim=int(args.embedding_dim), eval_steps=getattr(args, "eval_steps", 1),
                          seed=getattr(args, "seed", 0), num_nodes=num_nodes, step_every_epoch=step_every_epoch,
                          permutations=permutations, state_dict=state_dict, device=device, trace=trace)
    if not results["AUC"]:
        raise ValueError("no evaluation ran: args.epochs < 1")
    r = (100 * torch.tensor(results["AUC"])).numpy()
    return float(best_at_first_max(r)[1]), embs.cpu().clone().detach()


def reference_args(dataset, epochs=50, lr=0.01, embedding_dim=32, eval_steps=1, seed=1):
    """run_gic.py's DummyArgs fields CalGIC reads."""
    return SimpleNamespace(data_name=dataset, dataset=dataset, epochs=epochs, lr=lr, embedding_dim=embedding_dim,
                           eval_steps=eval_steps, log_steps=1, seed=seed, res_dir="")


def run_gic(split, data_name, runs=1, x=None, *, epochs=50, lr=0.01, embedding_dim=32, step_every_epoch=False,
            device=None):
    """The GIC row of Table 2 from a `workloads.Split` (run_gic.py: 50 epochs, lr 0.01, embedding 32, seed = run, x =
    None is eye(N)).  runs == 1: {'AUC': (best val, test at it), 'AP': (...)} as fractions, each chosen at the first
    evaluation of its own maximal val value; runs > 1: the list of those, one per run."""
    from .gae import _split_lists, best_at_first_max

    check_device(device)
    out = []
    for run in range(1, int(runs) + 1):
        results, _ = train(split.edge_index(), x, data_name, _split_lists(split), epochs=epochs, lr=lr,
                           embedding_dim=embedding_dim, eval_steps=1, seed=run, num_nodes=split.num_nodes,
                           step_every_epoch=step_every_epoch, device=device)
        if not results["AUC"]:
            raise ValueError("epochs must be >= 1")
        out.append({k: tuple(float(v) for v in best_at_first_max(np.asarray(r))) for k, r in results.items()})
    return out[0] if int(runs) == 1 else out
