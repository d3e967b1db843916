"""Subgraph sketching, the other scalable answer to SEAL (ELPH / BUDDY; Chamberlain et al., ICLR 2023): instead of
extracting a subgraph per link, every node's 0..k-hop ball gets a MinHash and a HyperLogLog sketch once, and the
structure counts that DRNL / DE labels would give are estimated per link from the two endpoints' sketches.  The
kernels are in csrc/s3grl_sketch.hip behind the C ABI s3grl_sketch_* and s3grl_masked_sketch_pairs; DESIGN.md §24 and
§25 are the specification (the reference has no BUDDY); tests/sketch_reference.py and tests/sketch_mask_reference.py
restate it in numpy.

    sk = SketchGraph(A, hops=2, num_perm=128, hll_p=8, seed=0)   # builds all hops on the device once
    sk.minhash, sk.hll            # [hops+1, N, P] int32 (the bit pattern of uint32), [hops+1, N, m] uint8, m = 2^hll_p
    sk.ball_sizes()               # fp32 [hops+1, N]: the estimated |B_i(v)|
    sk.intersections(links)       # fp32 [L, hops+1, hops+1]: I_ij, the estimated |B_i(u) ∩ B_j(v)|
    sk.features(links)            # fp32 [L, hops² + 2·hops] = [A_11..A_1k, …, A_kk | Bu_1..Bu_k | Bv_1..Bv_k]
    sk.raw(links)                 # (match int32, T int64, z int32), each [L, hops+1, hops+1]: the integers behind I
    sk.features(links, mask=True) # the same three calls with every link's own edge masked (hops <= 2)
    results = run_buddy(split, mask=True)   # {'AUC': (val, test), 'AP': (val, test)} of a BuddyTwin on the features

`A` is taken as `heuristics.canonical_csr` takes it and used structurally: row v's stored keys are N(v), values are
ignored and nothing is symmetrised.  A_ij estimates #{w: d(u,w) = i, d(v,w) = j}, Bu_i the nodes at distance i of u
and farther than `hops` from v.  The tables describe the graph as given.  By default a link's own edge stays in them,
so a train positive, an edge of the sketched graph, carries a mark that no test link has.  `mask=True` (ELPH's
answer) gives every link (u, v) the outputs of the graph without its own stored entries (u, v) and
(v, u): to the byte what `SketchGraph` of that smaller graph returns for the link, formed per link on the device from
the unmasked tables by a walk over the two endpoint rows.  A link that is no stored entry is unchanged.  That closed
form is exact for hops <= 2 only; `mask=True` with hops 3 or 4 raises NotImplementedError.

Everything on the hot path is integer min / max / compare / popcount, and the fp64 tail is single IEEE operations
in a fixed order: results are bit-identical across runs and link orders.  GPU only; there is no CPU fallback.  Node
ids outside [0, N) raise ValueError before any GPU work.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N
from .heuristics import canonical_csr, check_links

MAX_NODES, MAX_HOPS = 1 << 24, 4


def check_params(hops, num_perm, hll_p, seed):
    """(hops, num_perm, hll_p, seed) as the kernels take them; ValueError outside the envelope."""
    for name, x in (("hops", hops), ("num_perm", num_perm), ("hll_p", hll_p), ("seed", seed)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {x!r}")
    if not 1 <= hops <= MAX_HOPS:
        raise ValueError(f"need 1 <= hops <= {MAX_HOPS}, got {hops}")
    if not 64 <= num_perm <= 512 or num_perm % 64:
        raise ValueError(f"num_perm must be a multiple of 64 in [64, 512], got {num_perm}")
    if not 7 <= hll_p <= 10:
        raise ValueError(f"need 7 <= hll_p <= 10, got {hll_p}")
    if not 0 <= seed < 1 << 32:
        raise ValueError(f"seed must be a uint32, got {seed}")
    return int(hops), int(num_perm), int(hll_p), int(seed)


def check_graph(A):
    """The canonical CSR of `A`; ValueError unless 1 <= N <= 2^24 and nnz < 2^31 (beyond 2^24 nodes collisions of the
    32-bit hashes start to bias the estimates)."""
    A = canonical_csr(A)
    if not 1 <= A.shape[0] <= MAX_NODES or A.nnz >= 1 << 31:
        raise ValueError(f"need 1 <= N <= 2^24 and nnz < 2^31, got N = {A.shape[0]}, nnz = {A.nnz}")
    return A


def hll_constants(hll_p):
    """(m, C, LC) of DESIGN.md §24: C = α·m²·2^(33−p) with α = 0.7213 / (1 + 1.079 / m), and the linear-counting
    table LC[z] = m·ln(m / z) as m + 1 doubles (LC[0] = inf is never read), filled here so that the device
    evaluates no logarithm."""
    m = 1 << hll_p
    alpha = 0.7213 / (1.0 + 1.079 / m)
    LC = np.full(m + 1, np.inf)
    LC[1:] = m * np.log(m / np.arange(1, m + 1, dtype=np.float64))
    return m, alpha * m * m * 2.0 ** (33 - hll_p), LC


MASK_MAX_HOPS = 2


def check_mask(hops):
    """NotImplementedError unless masking a link's own edge is exact on the unmasked tables (hops <= 2)."""
    if hops > MASK_MAX_HOPS:
        raise NotImplementedError(
            f"mask=True needs hops <= {MASK_MAX_HOPS}, got {hops}: beyond that the rows of an endpoint's neighbours "
            "change too (a neighbour of u sees u's 1-ball without v), which a walk over the two endpoint rows "
            "cannot give")


class SketchGraph:
    """The MinHash and HyperLogLog sketches of every node's 0..hops-hop ball, built on the device once, with the
    per-link estimators on them.  Registered with its engine, which closes it."""

    def __init__(self, A, hops=2, num_perm=128, hll_p=8, seed=0, device=None):
        self.hops, self.num_perm, self.hll_p, self.seed = check_params(hops, num_perm, hll_p, seed)
        A = check_graph(A)
        if device is not None and torch.device(device).type == "cpu":
            raise RuntimeError("the sketches need a HIP device (MI355X); there is no CPU fallback")
        from .engine import default_engine

        self.engine = default_engine(device)
        dev = self.engine.device
        n = self.num_nodes = A.shape[0]
        self.num_registers, self._c, lc = hll_constants(self.hll_p)
        self._lc = torch.as_tensor(lc).to(dev)
        # the CSR stays on the device for the masked pairs kernel: (N + 1)·8 + nnz·4 bytes
        ip = self._indptr = torch.as_tensor(A.indptr.astype(np.int64)).to(dev)
        ix = self._indices = torch.as_tensor(A.indices.astype(np.int32)).to(dev)
        self.minhash = torch.empty((self.hops + 1, n, self.num_perm), dtype=torch.int32, device=dev)
        self.hll = torch.empty((self.hops + 1, n, self.num_registers), dtype=torch.uint8, device=dev)
        N.check(N.lib().s3grl_sketch_build(self.engine._ctx, n, N.ptr(ip), N.ptr(ix), int(A.nnz), self.hops,
                                           self.num_perm, self.hll_p, self.seed, N.ptr(self.minhash),
                                           N.ptr(self.hll)), "s3grl_sketch_build")
        torch.cuda.current_stream(dev).synchronize()
        self.engine._children.add(self)

    def ball_sizes(self):
        """fp32 [hops+1, N] on the device: the HyperLogLog estimate of |B_i(v)|."""
        self._alive()
        out = torch.empty((self.hops + 1, self.num_nodes), dtype=torch.float32, device=self.engine.device)
        N.check(N.lib().s3grl_sketch_cardinality(self.engine._ctx, self.hll_p, N.ptr(self._lc), self._c,
                                                 N.ptr(self.hll), out.numel(), N.ptr(out)), "s3grl_sketch_cardinality")
        return out

    def _pairs(self, links, want, mask=False):
        self._alive()
        if mask:
            check_mask(self.hops)
        ei = check_links(links, self.num_nodes)
        dev, L, K = self.engine.device, ei.shape[1], self.hops + 1
        shapes = {"match": ((L, K, K), torch.int32), "T": ((L, K, K), torch.int64), "z": ((L, K, K), torch.int32),
                  "intersections": ((L, K, K), torch.float32),
                  "features": ((L, self.hops * self.hops + 2 * self.hops), torch.float32)}
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in want}
        if L and mask:
            l_d = torch.as_tensor(ei.astype(np.int32)).to(dev).contiguous()
            N.check(N.lib().s3grl_masked_sketch_pairs(self.engine._ctx, self.num_nodes, N.ptr(self._indptr),
                                                      N.ptr(self._indices), self._indices.numel(), self.hops,
                                                      self.num_perm, self.hll_p, N.ptr(self.minhash), N.ptr(self.hll),
                                                      N.ptr(self._lc), self._c, N.ptr(l_d), L,
                                                      *(N.ptr(out.get(k)) for k in shapes)),
                    "s3grl_masked_sketch_pairs")
        elif L:
            l_d = torch.as_tensor(ei.astype(np.int32)).to(dev).contiguous()
            N.check(N.lib().s3grl_sketch_pairs(self.engine._ctx, self.num_nodes, self.hops, self.num_perm, self.hll_p,
                                               N.ptr(self.minhash), N.ptr(self.hll), N.ptr(self._lc), self._c,
                                               N.ptr(l_d), L, *(N.ptr(out.get(k)) for k in shapes)),
                    "s3grl_sketch_pairs")
        return out

    def features(self, links, mask=False):
        """The structure features of every link of `links` [2, L]: fp32 [L, hops² + 2·hops] on the device, laid out
        [A_11..A_1k, …, A_kk | Bu_1..Bu_k | Bv_1..Bv_k].  `mask=True`: of the graph without the link's own stored
        entries (hops <= 2, else NotImplementedError); by default the link's own edge stays in."""
        return self._pairs(links, ("features",), mask)["features"]

    def intersections(self, links, mask=False):
        """I_ij, the estimated |B_i(u) ∩ B_j(v)| of every link (u, v): fp32 [L, hops+1, hops+1] on the device.
        `mask` as for `features`."""
        return self._pairs(links, ("intersections",), mask)["intersections"]

    def raw(self, links, mask=False):
        """(match int32, T int64, z int32), each [L, hops+1, hops+1] on the device: the equal MinHash slots of
        (MH_i[u], MH_j[v]) and the register sum and zero count of max(HL_i[u], HL_j[v]).  `mask` as for `features`."""
        out = self._pairs(links, ("match", "T", "z"), mask)
        return out["match"], out["T"], out["z"]

    def _alive(self):
        if getattr(self, "minhash", None) is None:
            raise RuntimeError("SketchGraph is closed")

    def close(self):
        self.minhash = self.hll = self._lc = self._indptr = self._indices = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BuddyTwin(torch.nn.Module):
    """BUDDY's predictor: `label_lin` (Linear -> BatchNorm -> ReLU -> dropout) over the structure features, `feat_lin`
    (the same) over x_u ⊙ x_v when there are node features (num_features > 0), and a final Linear to one logit."""

    def __init__(self, num_features, hops, hidden=256, dropout=0.5):
        super().__init__()
        if isinstance(hops, bool) or not isinstance(hops, (int, np.integer)) or not 1 <= hops <= MAX_HOPS:
            raise ValueError(f"need 1 <= hops <= {MAX_HOPS}, got {hops!r}")
        if int(num_features) < 0 or int(hidden) < 1 or not 0.0 <= float(dropout) < 1.0:
            raise ValueError("need num_features >= 0, hidden >= 1 and 0 <= dropout < 1")
        self.num_features, self.hops, self.dropout = int(num_features), int(hops), float(dropout)
        dim = self.hops * self.hops + 2 * self.hops
        self.label_lin, self.label_bn = torch.nn.Linear(dim, hidden), torch.nn.BatchNorm1d(hidden)
        if self.num_features:
            self.feat_lin, self.feat_bn = torch.nn.Linear(self.num_features, hidden), torch.nn.BatchNorm1d(hidden)
        self.lin = torch.nn.Linear(hidden * (2 if self.num_features else 1), 1)

    def _branch(self, lin, bn, h):
        return torch.nn.functional.dropout(torch.relu(bn(lin(h))), self.dropout, self.training)

    def forward(self, structure, x_u=None, x_v=None):
        """structure fp32 [B, hops² + 2·hops]; x_u, x_v fp32 [B, num_features] when the model has features -> [B]."""
        h = self._branch(self.label_lin, self.label_bn, structure)
        if self.num_features:
            h = torch.cat([h, self._branch(self.feat_lin, self.feat_bn, x_u * x_v)], dim=1)
        return self.lin(h).reshape(-1)


def propagated_features(split, X, hops, device=None):
    """[X | ÂX | … | Â^hops X] fp32 [N, (hops+1)·F] on the device, Â the GCN operator of the split's training graph."""
    from .propagate import GcnGraph

    g = GcnGraph(split.edge_index(), split.num_nodes, device)
    x = torch.as_tensor(np.asarray(X, dtype=np.float32)).to(g.loc.device)
    if x.dim() != 2 or x.shape[0] != split.num_nodes:
        raise ValueError(f"X must be [{split.num_nodes}, F], got {tuple(x.shape)}")
    xs = [x]
    with torch.no_grad():
        for _ in range(hops):
            xs.append(g.propagate(xs[-1]))
    return torch.cat(xs, dim=1)


def train_buddy(model, structure, labels, x=None, links=None, *, epochs, lr, batch_size, seed, on_step=None):
    """Adam on BCE-with-logits over (structure [n, dim], labels [n]) in shuffled minibatches; `x` [N, F] and `links`
    [2, n] (device) feed the feature branch.  Returns the mean loss of every epoch; `on_step(loss)` sees each step's."""
    gen = torch.Generator(device="cpu").manual_seed(int(seed))
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    n, losses = structure.shape[0], []
    for _ in range(epochs):
        model.train()
        perm = torch.randperm(n, generator=gen).to(structure.device)
        total = 0.0
        for b0 in range(0, n, batch_size):
            at = perm[b0:b0 + batch_size]
            if at.numel() < 2:            # BatchNorm needs two rows
                continue
            opt.zero_grad()
            xu, xv = (x[links[0, at]], x[links[1, at]]) if x is not None else (None, None)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(model(structure[at], xu, xv), labels[at])
            loss.backward()
            opt.step()
            step = loss.item()
            if on_step is not None:
                on_step(step)
            total += step * at.numel()
        losses.append(total / n)
    return losses


def score_buddy(model, structure, x=None, links=None, batch_size=65536):
    model.eval()
    out = []
    with torch.no_grad():
        for b0 in range(0, structure.shape[0], batch_size):
            sl = slice(b0, b0 + batch_size)
            xu, xv = (x[links[0, sl]], x[links[1, sl]]) if x is not None else (None, None)
            out.append(model(structure[sl], xu, xv))
    return torch.cat(out) if out else torch.zeros(0, device=structure.device)


def run_buddy(split, hops=2, epochs=20, lr=0.01, seed=0, *, X=None, hidden=256, dropout=0.5, batch_size=1024,
              device=None, structure=None, history=None, sketch_seed=0, mask=False, **sketch_kwargs):
    """The BUDDY row from a `workloads.Split`: sketches of the train graph `split.A`, a `BuddyTwin` trained with BCE
    on the split's train positives / negatives, valid and test scored through `metrics.LinkMetrics`.  `X` [N, F]
    (optional) adds the feature branch over [X | ÂX | … | Â^hops X].  `structure` (optional) replaces the sketch
    features: a callable links [2, L] -> [L, hops² + 2·hops] (the probe trains on exact counts with it).  `history`,
    a list, receives every step's loss.  `seed` seeds the model and the shuffle, `sketch_seed` the hashes;
    `sketch_kwargs` are `SketchGraph`'s num_perm and hll_p.  `mask=True` featurises all six link lists with every
    link's own edge masked (`SketchGraph.features(links, mask=True)`; hops <= 2): only the train positives are
    entries of `split.A`, so only their rows change, and they lose the mark that no valid or test link carries.  It
    cannot be combined with `structure` (ValueError).  The feature branch is not masked: [X | ÂX | …] is propagated
    over the whole training graph.  Returns {'AUC': (val, test), 'AP': (val, test)}."""
    from .metrics import LinkMetrics

    check_params(hops, sketch_kwargs.get("num_perm", 128), sketch_kwargs.get("hll_p", 8), sketch_seed)
    if int(epochs) < 1 or not float(lr) > 0.0 or int(batch_size) < 2:
        raise ValueError("need epochs >= 1, lr > 0 and batch_size >= 2")
    if mask and structure is not None:
        raise ValueError("mask=True masks the sketch features; it cannot be combined with structure=")
    if mask:
        check_mask(hops)
    names = [("train", 0), ("train", 1), ("valid", 0), ("valid", 1), ("test", 0), ("test", 1)]
    lists = [check_links(split.links[s][k], split.num_nodes) for s, k in names]
    sk = SketchGraph(split.A, hops=hops, seed=sketch_seed, device=device, **sketch_kwargs)
    try:
        dev = sk.engine.device
        every = np.concatenate(lists, axis=1)
        feats = sk.features(every, mask=bool(mask)) if structure is None else \
            torch.as_tensor(np.asarray(structure(every), dtype=np.float32)).to(dev)
    finally:
        sk.close()
    links = torch.as_tensor(every).to(dev)
    x = propagated_features(split, X, hops, dev) if X is not None else None
    cuts = np.cumsum([0] + [a.shape[1] for a in lists])
    n_train = int(cuts[2])
    labels = torch.cat([torch.ones(int(cuts[1])), torch.zeros(n_train - int(cuts[1]))]).to(dev)
    torch.manual_seed(int(seed))
    model = BuddyTwin(0 if x is None else x.shape[1], hops, hidden, dropout).to(dev)
    train_buddy(model, feats[:n_train], labels, x, links[:, :n_train] if x is not None else None, epochs=int(epochs),
                lr=float(lr), batch_size=int(batch_size), seed=seed,
                on_step=history.append if history is not None else None)
    scores = score_buddy(model, feats[n_train:], x, links[:, n_train:] if x is not None else None)
    c = cuts[2:] - n_train
    m = LinkMetrics(dev)
    try:
        val = m.ranked(scores[c[0]:c[2]], n_pos=int(c[1] - c[0]))
        test = m.ranked(scores[c[2]:c[4]], n_pos=int(c[3] - c[2]))
    finally:
        m.close()
    return {"AUC": (val["AUC"], test["AUC"]), "AP": (val["AP"], test["AP"])}
