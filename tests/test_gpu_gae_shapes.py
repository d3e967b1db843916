"""The GAE kernels (csrc/s3grl_gae.hip) and the whole-graph GCN operator (gae.GcnGraph) where tests/test_gpu_gae.py does
not reach: every (VEC, LPD) lane layout of decode_kernel / backward_kernel, directed and irregular graphs through the
transposed operator, pair keys past 2^32, the exact selection rule of the negatives, incidence lists of tens of
thousands of entries, empty lists and awkward views of z.

Error bounds.  u = 2^-24.  A logit is a length-D fp32 sum: |err| <= 2·D·u·Σ_c |z_u,c · z_v,c|.  A gradient element is a
length-n sum over the node's n incidence entries: |err| <= 2·n·u·Σ_e |coef_e · z_other,c|, plus Σ_e coef_bound_e ·
|z_other,c| when the kernel computed coef itself.  Per-pair dL/dlogit (list length L, s = sigmoid(logit)): the logit's
error enters through |d coef / d logit| = s(1 − s) / L; the chain expf, 1 + e, 1 / ·, 1 − s, two products and a
quotient is under 9 roundings of quantities that are at most 1 / L in size (1 − s has an absolute error of 4u, which
the factor 1 / L scales; the quotient (1 − s) / (1 − s) of the negatives cancels it), taken as 16·u / L.  A loss term:
|d term / d logit| <= 1 times the logit bound, plus 3u + 2u·|term| for a positive and 4u·(1 + e^logit) + 2u·|term| for
a negative (−log(1 − s) divides the absolute error of 1 − s by 1 − s); the loss is the two means, plus 2u·|loss| for
the casts to fp32.  All of it comes from the fp64 restatement and the operands.  Every test prints its worst
error / bound; above 1 is a failure.  Logits are kept out of sigmoid's saturation by construction (`_fit`).
"""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import gae_reference as R
import seal_nn_reference as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = Path(__file__).resolve().parent / "golden"
U = 2.0 ** -24


def _rel(a, b):
    """tests/test_gpu_gae.py's figure: the error over the per-row (or per-list) maximum of the fp64 value."""
    a, b = a.double().cpu(), b.double().cpu()
    scale = b.abs().max(dim=-1, keepdim=True).values if b.dim() > 1 else b.abs().max()
    return float(((a - b).abs() / torch.clamp(scale, min=1e-30)).max())


# ---- error bounds from the fp64 restatement ------------------------------------------------------------------------
def _fit(z64, lists):
    """z as fp32 and as the fp64 reference of those fp32 values, rescaled by sqrt(8 / max|logit|) when a logit of
    `lists` passes 8; asserts max |logit| < 12 on the reference."""
    worst = max(float(R.logits(z64, p).abs().max()) for p in lists if p.shape[1])
    if worst > 8:
        z64 = z64 * math.sqrt(8 / worst)
    z32 = z64.float()
    zr = z32.double()
    assert max(float(R.logits(zr, p).abs().max()) for p in lists if p.shape[1]) < 12
    return z32, zr


def _ratio(got, ref, bound):
    """max |got − ref| / bound; where the bound is 0 the values must be equal."""
    err = (got.detach().double().cpu() - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    live = bound > 0
    return float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0


def _logit_bound(zr, pairs):
    return 2 * zr.shape[1] * U * (zr[pairs[0]].abs() * zr[pairs[1]].abs()).sum(dim=1)


def _coef_bound(zr, pairs):
    s = torch.sigmoid(R.logits(zr, pairs))
    L = max(pairs.shape[1], 1)
    return s * (1 - s) / L * _logit_bound(zr, pairs) + 16 * U / L


def _loss_bound(zr, pos, neg):
    xp, xn = R.logits(zr, pos), R.logits(zr, neg)
    tp, tn = -torch.log(torch.sigmoid(xp) + R.EPS), -torch.log(1 - torch.sigmoid(xn) + R.EPS)
    bp = _logit_bound(zr, pos) + 3 * U + 2 * U * tp
    bn = _logit_bound(zr, neg) + 4 * U * (1 + torch.exp(xn)) + 2 * U * tn
    return float(bp.mean() + bn.mean() + 2 * U * (tp.mean() + tn.mean()))


def _entries(lists, n):
    return sum(torch.bincount(p.reshape(-1), minlength=n) for p in lists)


def _grad_bound(zr, lists, coefs, coef_bounds=None):
    """Per element of grad_z: 2·n·u·Σ|coef·z_other| + Σ coef_bound·|z_other|."""
    n = zr.shape[0]
    mag = sum(R.pair_backward(zr.abs(), p, c.abs()) for p, c in zip(lists, coefs))
    b = 2 * _entries(lists, n)[:, None] * U * mag
    if coef_bounds is not None:
        b = b + sum(R.pair_backward(zr.abs(), p, cb) for p, cb in zip(lists, coef_bounds))
    return b


# ---- C.1 every lane layout ----------------------------------------------------------------------------------------
def lanes_rule(D):
    """s3grl_gae.hip's S3GRL_GAE_DISPATCH and lanes_for, restated: (VEC, LPD, trips of the channel loop)."""
    vec = 4 if D % 4 == 0 else 1
    lpd = 1
    while lpd < D // vec and lpd < 64:
        lpd *= 2
    return vec, lpd, -(-D // (lpd * vec))


# D -> (VEC, LPD, trips).  Ragged (D is no multiple of LPD · VEC, so some lanes of a group own no channel in the last
# trip): 3, 5, 12, 13, 17, 20, 33, 65, 260, 1000, 1028.
DIMS = {
    1: (1, 1, 1), 2: (1, 2, 1), 3: (1, 4, 1), 5: (1, 8, 1), 13: (1, 16, 1), 17: (1, 32, 1), 33: (1, 64, 1),
    65: (1, 64, 2),
    4: (4, 1, 1), 8: (4, 2, 1), 12: (4, 4, 1), 16: (4, 4, 1), 20: (4, 8, 1), 64: (4, 16, 1), 128: (4, 32, 1),
    256: (4, 64, 1), 260: (4, 64, 2), 512: (4, 64, 2), 1000: (4, 64, 4), 1028: (4, 64, 5),
}


def test_the_dimension_list_covers_every_lane_layout():
    assert {D: lanes_rule(D) for D in DIMS} == DIMS
    pairs = {(v, l) for v, l, _ in DIMS.values()}
    assert pairs == {(v, l) for v in (1, 4) for l in (1, 2, 4, 8, 16, 32, 64)} and len(pairs) == 14
    assert {v for v, l, t in DIMS.values() if t > 1} == {1, 4}            # a second trip with and without float4
    ragged = [D for D, (v, l, t) in DIMS.items() if D % (l * v)]
    assert sorted(ragged) == [3, 5, 12, 13, 17, 20, 33, 65, 260, 1000, 1028]
    assert any(DIMS[D][0] == 4 for D in ragged) and any(DIMS[D][0] == 1 for D in ragged)
    assert any(DIMS[D][2] > 1 for D in ragged)


N_HUB = 203                                   # not a multiple of the 4 nodes of a backward block
ISOLATED = [5, 77, N_HUB - 2, N_HUB - 1]      # in no pair of either list


def _hub_list(rng, live, hub, noise, selfs, dups):
    v = rng.choice(live, hub)
    w = rng.choice(live, hub)
    s = rng.choice(live[live != 0], selfs)
    p = np.concatenate([np.stack([np.zeros(hub, dtype=np.int64), v]), np.stack([w, np.zeros(hub, dtype=np.int64)]),
                        rng.choice(live, (2, noise)), np.stack([s, s])], axis=1)
    p = np.concatenate([p, p[:, rng.choice(p.shape[1], dups)]], axis=1)
    return torch.as_tensor(p[:, rng.permutation(p.shape[1])])


@pytest.fixture(scope="module")
def hub_lists():
    rng = np.random.default_rng(11)
    live = np.setdiff1d(np.arange(N_HUB), ISOLATED)
    pos, neg = _hub_list(rng, live, 700, 1500, 20, 100), _hub_list(rng, live, 300, 1000, 5, 30)
    for p in (pos, neg):
        assert int((p[0] == p[1]).sum()) >= 5                               # self pairs
        assert np.unique(p.numpy(), axis=1).shape[1] < p.shape[1]           # duplicated pairs
        assert int(_entries([p], N_HUB)[0]) >= 600                          # the hub
    assert not _entries([pos, neg], N_HUB)[ISOLATED].any()
    return pos, neg


def _run_lists(z32, pos, neg, w):
    """Everything the pair kernels give for z on fresh PairLists: logits, coef, loss, d recon_loss / dz,
    d <w, decode(pos)> / dz."""
    from s3grl_amd import gae

    n = z32.shape[0]
    z = z32.to(DEV).requires_grad_(True)
    pos_l, neg_l = gae.PairList(pos, n, DEV), gae.PairList(neg, n, DEV)
    logits, coef, loss = gae._decode(z.detach(), pos_l, neg_l, loss=True)
    out = gae.recon_loss(z, pos_l, neg_l)
    (g_loss,) = torch.autograd.grad(out, z)
    lg = gae.inner_product_decode(z, pos_l)
    (g_dec,) = torch.autograd.grad(lg, z, w.to(DEV))
    return [t.detach().cpu() for t in (logits, coef, loss.view(()), out, g_loss, lg, g_dec)]


def _check_lists(z64, pos, neg, seed, tag, rel=None, twice=True):
    """The pair kernels on (z, pos, neg) against fp64, within the bounds of the module docstring; twice, bit-equal."""
    n, P = z64.shape[0], pos.shape[1]
    z32, zr = _fit(z64, [pos, neg])
    w = torch.randn(P, generator=torch.Generator().manual_seed(seed))
    first = _run_lists(z32, pos, neg, w)
    logits, coef, loss, out, g_loss, lg, g_dec = first
    both = torch.cat([pos, neg], dim=1)
    ref_logits = R.logits(zr, both)
    ref_coef = R.recon_coef(zr, pos, neg)
    cb = torch.cat([_coef_bound(zr, pos), _coef_bound(zr, neg)])
    za = zr.clone().requires_grad_(True)
    ref_loss = R.recon_loss(za, pos, neg)
    (ref_g,) = torch.autograd.grad(ref_loss, za)
    ref_loss = ref_loss.detach()
    ratios = {
        "logit": _ratio(logits, ref_logits, _logit_bound(zr, both)),
        "coef": _ratio(coef, ref_coef, cb),
        "loss": abs(float(loss) - float(ref_loss)) / _loss_bound(zr, pos, neg),
        "grad": _ratio(g_loss, ref_g, _grad_bound(zr, [pos, neg], [ref_coef[:P], ref_coef[P:]], [cb[:P], cb[P:]])),
        "decode_grad": _ratio(g_dec, R.pair_backward(zr, pos, w.double()), _grad_bound(zr, [pos], [w.double()])),
    }
    print(f"{tag}: error / bound " + ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert torch.equal(out, loss) and torch.equal(lg, logits[:P])
    assert all(v <= 1 for v in ratios.values()), ratios
    zero = torch.zeros(z32.shape[1])
    for i in torch.nonzero(_entries([pos, neg], n) == 0).flatten().tolist():
        assert torch.equal(g_loss[i], zero) and torch.equal(g_dec[i], zero)
    for i in torch.nonzero(_entries([pos], n) == 0).flatten().tolist():
        assert torch.equal(g_dec[i], zero)
    if rel is not None:                                                     # the suite's figure where it was set
        assert _rel(logits, ref_logits) < rel and _rel(coef, ref_coef) < rel and _rel(g_loss, ref_g) < rel
        assert abs(float(loss) - float(ref_loss)) <= rel * abs(float(ref_loss))
    for a, b in zip(first, _run_lists(z32, pos, neg, w) if twice else ()):  # determinism
        assert torch.equal(a, b)
    return ratios, (g_loss, ref_g)


@pytest.mark.parametrize("D", sorted(DIMS))
def test_pair_kernels_at_every_lane_layout(hub_lists, D):
    pos, neg = hub_lists
    z64 = torch.randn((N_HUB, D), generator=torch.Generator().manual_seed(D), dtype=torch.float64) * D ** -0.25
    _check_lists(z64, pos, neg, D, f"D={D} {lanes_rule(D)}", rel=1e-5 if D <= 32 else None)


# ---- C.2 / C.3 directed and irregular whole-graph propagation -----------------------------------------------------
def _usair_arcs():
    lab = np.load(GOLDEN / "labels_directed_usair.npz")
    return int(lab["num_nodes"]), torch.as_tensor(lab["arcs"].T.astype(np.int64))


def _irregular_arcs():
    """400 nodes: 0..39 have no in-arc, 40..79 no out-arc, 80..98 no arc at all, 99 only an input self-loop; the
    rest random, with input self-loops and duplicated arcs (self-loops among them)."""
    rng = np.random.default_rng(3)
    rest = np.arange(100, 400)
    src = rng.choice(np.concatenate([np.arange(0, 40), rest]), 2500)
    dst = rng.choice(np.concatenate([np.arange(40, 80), rest]), 2500)
    loops = np.concatenate([rng.choice(rest, 30, replace=False), [99]])
    a = np.concatenate([np.stack([src, dst]), np.stack([loops, loops])], axis=1)
    a = np.concatenate([a, a[:, rng.choice(a.shape[1], 200)], np.stack([loops[:5], loops[:5]])], axis=1)
    ei = torch.as_tensor(a[:, rng.permutation(a.shape[1])])
    assert not np.isin(a[1], np.arange(0, 40)).any() and not np.isin(a[0], np.arange(40, 80)).any()
    assert not np.isin(a, np.arange(80, 99)).any()
    assert int((ei[0] == ei[1]).sum()) >= 36 and np.unique(a, axis=1).shape[1] < a.shape[1]
    return 400, ei


GRAPHS = {"usair_directed": _usair_arcs, "irregular": _irregular_arcs}


def _assert_asymmetric(ei):
    arcs = set(zip(ei[0].tolist(), ei[1].tolist()))
    assert sum((v, u) not in arcs for u, v in arcs) > len(arcs) // 4        # really directed


@pytest.mark.parametrize("H", [1, 24, 37, 64, 256])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_directed_whole_graph_propagation_forward_and_backward(name, H):
    from s3grl_amd import gae

    n, ei = GRAPHS[name]()
    _assert_asymmetric(ei)
    graph = gae.GcnGraph(ei, n, DEV)
    g = torch.Generator().manual_seed(H)
    h = torch.randn((n, H), generator=g).to(DEV).requires_grad_()
    bias = torch.randn(H, generator=g).to(DEV).requires_grad_()
    out = graph.propagate(h, bias)
    gout = torch.randn((n, H), generator=g).to(DEV)
    gh, gb = torch.autograd.grad(out, (h, bias), gout)
    src, dst, coef = SR.gcn_norm(ei, n)
    ref = SR.propagate(h.detach().double().cpu(), src, dst, coef) + bias.detach().double().cpu()
    ref_gh = SR.propagate(gout.double().cpu(), dst, src, coef)
    wrong = SR.propagate(gout.double().cpu(), src, dst, coef)               # the forward operator: not the gradient
    assert float((ref_gh - wrong).abs().max()) > 1e-2
    torch.testing.assert_close(out.double().cpu(), ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gh.double().cpu(), ref_gh, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gb.double().cpu(), gout.double().cpu().sum(0), rtol=1e-5, atol=1e-5)
    out2 = graph.propagate(h, bias)
    assert torch.equal(out, out2) and torch.equal(gh, torch.autograd.grad(out2, h, gout)[0])


@pytest.mark.parametrize("model", ["GAE", "VGAE"])
def test_teacher_forced_step_on_a_directed_graph(model):
    from s3grl_amd import gae

    n, ei = _usair_arcs()
    _assert_asymmetric(ei)
    net = gae.TWINS[model](n, 32, 64, seed=4).to(DEV)
    net.train()
    graph, pos = gae.GcnGraph(ei, n, DEV), gae.PairList(ei, n, DEV)
    neg = gae.recon_negatives(pos, 5, 1)
    noise = 0.1 * torch.randn((n, 32), generator=torch.Generator().manual_seed(3)) if net.variational else None
    z = net.encode(None, graph, noise=None if noise is None else noise.to(DEV))
    loss = net.recon_loss(z, pos, neg)
    loss.backward()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    ref_loss, grads = R.step(sd, None, ei, n, model, neg.edge_index().cpu(), noise)
    assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-4 * abs(float(ref_loss))
    params = dict(net.named_parameters())
    for name, g in grads.items():
        assert _rel(params[name].grad, g) < 1e-4, name


# ---- C.4 keys past 2^32 -------------------------------------------------------------------------------------------
N_BIG = 70_000


@pytest.fixture(scope="module")
def big_graph():
    rng = np.random.default_rng(2)
    e = rng.integers(0, N_BIG, size=(2, 101_000))
    e = e[:, e[0] != e[1]]
    e = np.unique(np.concatenate([e, e[::-1]], axis=1), axis=1)             # both directions, no duplicates
    return torch.as_tensor(e[:, rng.permutation(e.shape[1])])


def _sampled_keys(pos_l, count, seed, epoch):
    from s3grl_amd import gae

    neg = gae._sample(pos_l, count, seed, epoch)
    return neg, R.pair_key(neg.src.long().cpu(), neg.dst.long().cpu(), pos_l.num_nodes)


def test_keys_and_negatives_past_32_bits(big_graph):
    from s3grl_amd import gae

    ei, n = big_graph, N_BIG
    assert 195_000 < ei.shape[1] < 205_000 and n * (n - 1) > 2 ** 32
    pos_l = gae.PairList(ei, n, DEV)
    keys, m = pos_l.keys()
    want = torch.sort(R.pair_key(ei[0], ei[1], n)).values
    assert m == ei.shape[1] and torch.equal(keys.cpu(), want)
    assert int((want >= 2 ** 32).sum()) > 1000 and int((want < 2 ** 32).sum()) > 1000
    lists = []
    for count, seed, epoch in ((5_000, 3, 2), (m + n, 5, 1)):                # below, and PyG's default
        trace = {}
        ref = R.negatives(want.numpy(), n, count, seed, epoch, trace)
        neg, got = _sampled_keys(pos_l, count, seed, epoch)
        assert not trace["enumerate"] and len(ref) == count
        assert torch.equal(got, ref)                                        # the same pairs in the same order
        i, j = R.pair_of_key(ref, n)
        assert torch.equal(neg.src.long().cpu(), i) and torch.equal(neg.dst.long().cpu(), j)
        assert int((got >= 2 ** 32).sum()) > count // 100 and int(got.max()) > 2 ** 32
        lists.append(neg.edge_index().cpu())
    z64 = torch.randn((n, 32), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 0.4
    _check_lists(z64, ei, lists[1], 7, "N=70000 D=32", twice=False)


# ---- C.5 the selection rule, exactly ------------------------------------------------------------------------------
def _usair_train():
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    s = W.edge_split(n, e, seed=0)
    return s.num_nodes, torch.as_tensor(s.edge_index())


def test_negatives_equal_the_restatement_on_usair():
    from s3grl_amd import gae

    n, ei = _usair_train()
    pos_l = gae.PairList(ei, n, DEV)
    keys, m = pos_l.keys()
    pos_keys = keys.cpu().numpy()[:m]
    assert np.array_equal(pos_keys, np.sort(R.pair_key(ei[0], ei[1], n).numpy()))
    for seed, epoch, count in ((7, 1, 1), (7, 1, 50), (7, 2, 50), (3, 0, m), (1, 50, m + n), (2 ** 33 + 9, 4, m + n)):
        trace = {}
        ref = R.negatives(pos_keys, n, count, seed, epoch, trace)
        _, got = _sampled_keys(pos_l, count, seed, epoch)
        assert len(ref) == count and torch.equal(got, ref), (seed, epoch, count)
        assert trace["kept_per_round"][0] == count                          # round 1 suffices, and is cut at `count`
        assert count == 1 or int(ref.max()) > n * (n - 1) // 2              # cut in draw order, not at the small keys


def test_negatives_when_round_one_falls_short():
    from s3grl_amd import gae

    n = 40
    rng = np.random.default_rng(4)
    pop = n * (n - 1)
    pos_keys = torch.as_tensor(np.sort(rng.choice(pop, 936, replace=False)))      # 60 % of the ordered pairs
    i, j = R.pair_of_key(pos_keys, n)
    pos_l = gae.PairList(torch.stack([i, j])[:, torch.as_tensor(rng.permutation(936))], n, DEV)
    free = pop - 936
    seen = set()
    for count in (free // 2, (9 * free) // 10):
        for seed, epoch in ((0, 0), (1, 3), (2, 7)):
            trace = {}
            ref = R.negatives(pos_keys.numpy(), n, count, seed, epoch, trace)
            _, got = _sampled_keys(pos_l, count, seed, epoch)
            assert torch.equal(got, ref), (count, seed, epoch)
            kept = trace["kept_per_round"]
            assert not trace["enumerate"] and kept[0] < count and kept[1] > 0     # round 1 fell short
            seen.add("filled" if len(ref) == count else "short")
            if count == free // 2:
                assert len(ref) == count and sum(kept) == count
    print("round-1-short cases:", sorted(seen))
    assert "filled" in seen


def test_negatives_either_side_of_the_enumerate_threshold():
    from s3grl_amd import gae

    n = 12
    ring = torch.tensor([[i, (i + 1) % n] for i in range(n)] + [[(i + 1) % n, i] for i in range(n)]).T
    pos_l = gae.PairList(ring, n, DEV)
    pos_keys = torch.sort(R.pair_key(ring[0], ring[1], n)).values
    pop = n * (n - 1)
    free = np.setdiff1d(np.arange(pop), pos_keys.numpy())
    modes = {}
    for count in (98, 99):                                       # 1.1·count / (1 − 24/132) = 131.8 and 133.1; pop = 132
        for seed, epoch in ((0, 0), (6, 2)):
            trace = {}
            ref = R.negatives(pos_keys.numpy(), n, count, seed, epoch, trace)
            _, got = _sampled_keys(pos_l, count, seed, epoch)
            assert torch.equal(got, ref), (count, seed, epoch)
            modes[count] = trace["S"]
            if trace["S"] == pop:
                assert trace["enumerate"] and got.tolist() == free[:count].tolist()
    assert modes[98] == 131 < pop and modes[99] == pop          # one ran in each mode


# ---- C.6 long incidence lists -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def star_lists():
    n = 1500
    rng = np.random.default_rng(8)

    def star(hub, noise):
        z = np.zeros(hub, dtype=np.int64)
        p = np.concatenate([np.stack([z, rng.integers(1, n, hub)]), np.stack([rng.integers(1, n, hub), z]),
                            rng.integers(0, n, (2, noise))], axis=1)
        return torch.as_tensor(p[:, rng.permutation(p.shape[1])])

    pos, neg = star(26_000, 4_000), star(3_000, 4_000)
    assert int((pos[0] == 0).sum()) >= 26_000 and int((pos[1] == 0).sum()) >= 26_000
    assert int(_entries([pos, neg], n)[0]) >= 58_000 and int(_entries([pos], n)[0]) >= 52_000
    return n, pos, neg


@pytest.mark.parametrize("D", [4, 32, 256])
def test_hub_with_tens_of_thousands_of_entries(star_lists, D):
    n, pos, neg = star_lists
    z64 = torch.randn((n, D), generator=torch.Generator().manual_seed(100 + D), dtype=torch.float64) * D ** -0.25
    ratios, (g, ref_g) = _check_lists(z64, pos, neg, D, f"star D={D}")
    print(f"star D={D}: hub row error / row max {float((g[0].double() - ref_g[0]).abs().max() / ref_g[0].abs().max()):.3g}")


# ---- C.7 empty and awkward inputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("empty", ["neg", "pos"])
def test_an_empty_list_gives_nan_loss_and_the_other_lists_gradient(hub_lists, empty):
    from s3grl_amd import gae

    full = hub_lists[0]
    none = torch.zeros((2, 0), dtype=torch.int64)
    pos, neg = (full, none) if empty == "neg" else (none, full)
    z64 = torch.randn((N_HUB, 20), generator=torch.Generator().manual_seed(9), dtype=torch.float64) * 0.4
    z32, zr = _fit(z64, [full])
    z = z32.to(DEV).requires_grad_(True)
    out = gae.recon_loss(z, pos, neg)
    assert out.shape == () and math.isnan(float(out.detach()))
    out.backward()
    za = zr.clone().requires_grad_(True)
    ref = R.recon_loss(za, pos, neg)
    assert math.isnan(float(ref.detach()))
    ref.backward()
    assert bool(torch.isfinite(za.grad).all()) and float(za.grad.abs().max()) > 0    # what fp64 autograd gives
    coef = R.recon_coef(zr, pos, neg)
    r = _ratio(z.grad, za.grad, _grad_bound(zr, [full], [coef], [_coef_bound(zr, full)]))
    print(f"empty {empty}: grad error / bound {r:.3g}")
    assert r <= 1
    for i in ISOLATED:
        assert torch.equal(z.grad[i].cpu(), torch.zeros(20))


def test_awkward_views_of_z_give_the_bits_of_the_contiguous_copy(hub_lists):
    from s3grl_amd import gae

    pos, neg = hub_lists
    D = 20
    z32, _ = _fit(torch.randn((N_HUB, D), generator=torch.Generator().manual_seed(10), dtype=torch.float64) * 0.4,
                  [pos, neg])
    base = z32.to(DEV)
    assert base.data_ptr() % 16 == 0
    transposed = base.t().contiguous().t()
    flat = torch.zeros(N_HUB * D + 1, device=DEV)
    flat[1:] = base.reshape(-1)
    shifted = flat[1:].view(N_HUB, D)
    assert not transposed.is_contiguous() and shifted.is_contiguous() and shifted.data_ptr() % 16 == 4
    assert torch.equal(transposed, base) and torch.equal(shifted, base)
    w = torch.randn(pos.shape[1], generator=torch.Generator().manual_seed(1)).to(DEV)
    pos_l, neg_l = gae.PairList(pos, N_HUB, DEV), gae.PairList(neg, N_HUB, DEV)

    def run(view):
        z = view.detach().requires_grad_(True)                              # keeps the strides and the offset
        assert z.stride() == view.stride() and z.data_ptr() == view.data_ptr()
        loss = gae.recon_loss(z, pos_l, neg_l)
        (g1,) = torch.autograd.grad(loss, z)
        lg = gae.inner_product_decode(z, pos_l)
        (g2,) = torch.autograd.grad(lg, z, w)
        return loss.detach(), g1, lg.detach(), g2

    want = run(base.clone())
    for view in (transposed, shifted):
        for a, b in zip(want, run(view)):
            assert a.shape == b.shape and torch.equal(a, b)
