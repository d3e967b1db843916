"""Raw-edge message passing on the MI355X: s3grl_amd.mpnn / mpgnn against the fp64 restatement
(tests/mpnn_reference.py) under forward-error bounds computed from the restatement alone, bit-identical repeats,
the twins' logits and gradients, and end-to-end training.

Aggregation bound, for a row with d entries:  |out - ref| <= (d + 3) · 2^-24 · (|self_coef·h_i| + Σ_e |s(e)·h_j|):
one rounding per add, one for the scale product, one for the self term, one for 1 / deg in fp32.
Segment mean bound, for a graph of n rows:  (n + 2) · 2^-24 · Σ|x| / n."""
import numpy as np
import pytest
import torch

from conftest import csr_from_arcs
from mpnn_reference import (aggregate_mean, aggregate_mean_t, aggregate_mean_t_wrong_side, aggregate_sum,
                            aggregate_sum_t, gin_forward, in_degree, net_forward, sage_forward, segment_mean,
                            torch_operators)

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd.engine import Engine

    e = Engine("cuda:0")
    yield e
    e.close()


def _split(name, seed=0):
    from s3grl_amd import workloads as W

    n, e = W.load_topology(name)
    return W.edge_split(n, e, seed=seed)


def subgraphs(eng, li, A, hops, label, x=None, **kw):
    from s3grl_amd.seal import enclosing_subgraphs

    return enclosing_subgraphs(np.asarray(li), A, x, 0, hops, label, engine=eng, **kw)


@pytest.fixture(scope="module")
def usair600(eng):
    """The first 600 USAir 2-hop links of the split test_gpu_seal_nn.py uses."""
    sp = _split("usair")
    li, _ = sp.all_links()
    return subgraphs(eng, li[:, :600], sp.A, 2, "drnl")


def _ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the result must be exact."""
    err = (got.double() - ref).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "a row with a zero bound is not exact"
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def check_aggregate(op, edge_index, H, mode, self_coef, seed=0):
    """Forward and backward of aggregate(h, op, mode, self_coef) against the restatement on `edge_index`; returns the
    worst error / bound ratios (forward, backward), both asserted <= 1."""
    from s3grl_amd.mpnn import aggregate

    n = op.num_nodes
    src, dst = edge_index[0], edge_index[1]
    g = torch.Generator(device="cuda").manual_seed(seed)
    h = torch.randn((n, H), device="cuda", generator=g).requires_grad_()
    out = aggregate(h, op, mode, self_coef)
    gout = torch.randn((n, H), device="cuda", generator=g)
    (gh,) = torch.autograd.grad(out, h, gout)
    hd, gd = h.detach().double(), gout.double()
    fwd, bwd = (aggregate_mean, aggregate_mean_t) if mode == "mean" else (aggregate_sum, aggregate_sum_t)
    d_in = in_degree(dst, n)[:, None]
    d_out = in_degree(src, n)[:, None]
    ref = self_coef * hd + fwd(hd, src, dst)
    bound = (d_in + 3) * U * ((self_coef * hd).abs() + fwd(hd.abs(), src, dst))
    ref_g = self_coef * gd + bwd(gd, src, dst)
    bound_g = (d_out + 3) * U * ((self_coef * gd).abs() + bwd(gd.abs(), src, dst))
    r = _ratio(out.detach(), ref, bound), _ratio(gh, ref_g, bound_g)
    assert max(r) <= 1.0, (mode, self_coef, H, r)
    return r


@pytest.mark.parametrize("H", [1, 3, 4, 32, 37, 256, 257, 260])
def test_aggregate_every_layout_on_usair(usair600, H):
    """Both VEC paths at (VEC, LPN) = (1,1), (1,4), (4,1), (4,8), (1,64), (4,64), a second trip of the channel loop
    with and without float4; sum (no scale, both passes), mean (OWN forward, NEIGHBOUR backward); self_coef 0, 1, 1.25;
    rows the identity and a shuffled subset.  Not every layout: LPN 2, 16, 32 and (1,8), (4,2), (4,4) run in
    test_gpu_subgraph_ops.py, whose sweep reaches all 14."""
    subs = usair600
    worst = 0.0
    for ids in (np.arange(600), np.random.default_rng(5).permutation(600)[:300]):
        b = subs.batch(ids)
        assert (ids.size == 600) == bool(torch.equal(b.rows, torch.arange(b.num_nodes, device="cuda")))
        ei = b.edge_index
        for mode in ("sum", "mean"):
            for self_coef in (0.0, 1.0, 1.25):
                worst = max(worst, *check_aggregate(b, ei, H, mode, self_coef, seed=H))
    print(f"[mpnn] aggregate H = {H}: worst error / bound {worst:.3f}")


def directed400():
    """400 nodes: every in-degree 0..9 (node i < 360 has i % 10), sources drawn from 0..339 only, so 340..359 are
    sinks without out-arcs and 360..399 isolated; some input self-loops and duplicated arcs are forced."""
    rng = np.random.default_rng(17)
    arcs = []
    for i in range(360):
        k = i % 10
        s = rng.integers(0, 340, size=k)
        if k >= 2 and i % 7 == 0:
            s[1] = s[0]                       # a duplicated arc
        if k >= 1 and i % 11 == 0 and i < 340:
            s[0] = i                          # an input self-loop
        arcs += [(int(j), i) for j in s]
    return 400, np.asarray(arcs, dtype=np.int64)


def test_directed_graph_whole_and_as_subgraphs(eng):
    from s3grl_amd.mpnn import NbrGraph, aggregate

    n, arcs = directed400()
    ei = torch.as_tensor(arcs.T.copy()).cuda()
    src, dst = ei[0], ei[1]
    d_in, d_out = in_degree(dst, n), in_degree(src, n)
    assert sorted(set(d_in.long().tolist())) == list(range(10))          # every remainder of the unrolled walk
    assert bool((src == dst).any())                                        # input self-loops
    assert torch.unique(src * n + dst).numel() < src.numel()               # duplicated arcs
    assert bool(((d_in == 0) & (d_out > 0)).any()) and bool(((d_out == 0) & (d_in > 0)).any())
    isolated = (d_in == 0) & (d_out == 0)
    assert int(isolated.sum()) >= 40
    graph = NbrGraph(ei, n)
    worst = 0.0
    for H in (1, 4, 32):
        for mode in ("sum", "mean"):
            for self_coef in (0.0, 1.25):
                worst = max(worst, *check_aggregate(graph, ei, H, mode, self_coef, seed=3))
    g = torch.Generator(device="cuda").manual_seed(4)
    h = torch.randn((n, 32), device="cuda", generator=g).requires_grad_()
    out = aggregate(h, graph, "mean")
    assert bool((out[isolated] == 0).all()) and bool((out[d_in == 0] == 0).all())   # zero rows, never NaN
    gout = torch.randn_like(out)
    (gh,) = torch.autograd.grad(out, h, gout)
    gd = gout.double()
    # the graph tells the transposed operator from the forward one, and the scale's two sides apart
    bound = (d_out[:, None] + 3) * U * aggregate_mean_t(gd.abs(), src, dst)
    assert bool(((gh.double() - aggregate_mean(gd, src, dst)).abs() > bound + 1e-3).any())
    assert bool(((aggregate_mean_t_wrong_side(gd, src, dst) - aggregate_mean_t(gd, src, dst)).abs() > 1e-3).any())
    assert bool(((gh.double() - aggregate_mean_t_wrong_side(gd, src, dst)).abs() > 1e-3).any())
    # the same graph through SEAL: directed 2-hop subgraphs (self-loops kept, duplicates merged by the CSR)
    A = csr_from_arcs(n, arcs)
    A.sum_duplicates()
    A.data[:] = 1
    links = np.stack([np.arange(0, 80, 2), np.arange(100, 180, 2)])
    subs = subgraphs(eng, links, A, 2, "drnl", directed=True)
    b = subs.batch(np.arange(len(subs))[::-1].copy())
    bei = b.edge_index
    assert bool((bei[0] == bei[1]).any())
    pairs = set(zip(bei[0].tolist(), bei[1].tolist()))
    assert any((v, u) not in pairs for u, v in pairs)                      # really directed
    for H in (3, 32):
        for mode in ("sum", "mean"):
            worst = max(worst, *check_aggregate(b, bei, H, mode, 1.0, seed=6))
    print(f"[mpnn] directed 400-node graph: worst error / bound {worst:.3f}")


def test_edge_weight_and_raw_instances_agree_bit_for_bit(eng):
    """s3grl_gcn_propagate and s3grl_nbr_aggregate are instances of one kernel: on one CSR, a per-entry coefficient of
    1 is the raw sum (fma(1, v, acc) = acc + v exactly) and coef[e] = scale[nbr[e]] is the NEIGHBOUR side.  H covers
    both VEC paths, LPN 1, 4 and 64, and a second trip of the channel loop with and without float4; the graph has every
    in-degree 0..9, so every remainder of the unrolled walk and the empty row."""
    import ctypes as C

    from s3grl_amd import _native as N
    from s3grl_amd.mpnn import NbrGraph

    def p(t):
        return C.c_void_p(t.data_ptr() if t is not None else 0)

    n, arcs = directed400()
    graph = NbrGraph(torch.as_tensor(arcs.T.copy()).cuda(), n)
    E = graph.in_nbr.numel()
    g = torch.Generator(device="cuda").manual_seed(9)
    for H in (1, 3, 4, 37, 260):
        h = torch.randn((n, H), device="cuda", generator=g)

        def edge(coef):
            out = torch.empty_like(h)
            N.check(N.lib().s3grl_gcn_propagate(eng._ctx, n, H, p(graph.rows), p(graph.loc), p(graph.in_ptr),
                                                p(graph.in_nbr), p(coef), p(h), p(None), p(out)), "s3grl_gcn_propagate")
            return out

        def raw(scale, side):
            out = torch.empty_like(h)
            N.check(N.lib().s3grl_nbr_aggregate(eng._ctx, n, H, p(graph.rows), p(graph.loc), p(graph.in_ptr),
                                                p(graph.in_nbr), p(scale), side, 0.0, p(h), p(out)),
                    "s3grl_nbr_aggregate")
            return out

        assert torch.equal(edge(torch.ones(E, device="cuda")), raw(None, N.SCALE_NONE)), H
        assert torch.equal(edge(graph.scale[graph.in_nbr.long()].contiguous()), raw(graph.scale, N.SCALE_NEIGHBOUR)), H


@pytest.mark.parametrize("H", [4, 32])
def test_star_with_70000_leaves(eng, H):
    from s3grl_amd.mpnn import NbrGraph

    L = 70000
    leaves = torch.arange(1, L + 1)
    hub = torch.zeros(L, dtype=torch.int64)
    ei = torch.cat([torch.stack([leaves, hub]), torch.stack([hub, leaves])], 1).cuda()
    graph = NbrGraph(ei, L + 1)
    worst = 0.0
    for mode in ("sum", "mean"):
        worst = max(worst, *check_aggregate(graph, ei, H, mode, 1.0, seed=8))   # every row, the hub's among them
    print(f"[mpnn] star, H = {H}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("W", [1, 97, 128])
def test_segment_mean_sizes(eng, W):
    from s3grl_amd.mpnn import segment_mean as hip_segment_mean

    sizes = [1, 2, 63, 64, 65, 1000, 0, 70000, 3]
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.as_tensor(sizes), 0)
    g = torch.Generator(device="cuda").manual_seed(W)
    x = torch.randn((int(ptr[-1]), W), device="cuda", generator=g).requires_grad_()
    n = torch.as_tensor(sizes, dtype=torch.float64, device="cuda")[:, None]
    worst = 0.0
    for p, xs in ((ptr, x), (ptr[:8], x[:int(ptr[7])])):                  # with the long graph (chunked) and without
        nn_ = n[:p.numel() - 1]
        out = hip_segment_mean(xs, p.cuda())
        xd = xs.detach().double()
        ref = segment_mean(xd, p)
        bound = (nn_ + 2) * U * segment_mean(xd.abs(), p)
        worst = max(worst, _ratio(out.detach(), ref, bound))
        assert bool((out[6] == 0).all())                                   # the empty graph: a zero row
        gout = torch.randn_like(out)
        (gx,) = torch.autograd.grad(out, xs, gout)
        graph = torch.repeat_interleave(torch.arange(p.numel() - 1, device="cuda"), p.diff().cuda())
        ref_g = (gout.double() / nn_.clamp(min=1))[graph]
        worst = max(worst, _ratio(gx, ref_g, U * ref_g.abs()))            # one division, one rounding
    assert worst <= 1.0, worst
    print(f"[mpnn] segment mean W = {W}: worst error / bound {worst:.3f}")


def test_determinism(usair600):
    from s3grl_amd.mpnn import aggregate
    from s3grl_amd.mpnn import segment_mean as hip_segment_mean

    b = usair600.batch(np.arange(600))
    runs = []
    for _ in range(2):
        g = torch.Generator(device="cuda").manual_seed(11)
        h = torch.randn((b.num_nodes, 97), device="cuda", generator=g).requires_grad_()
        outs = []
        for mode, coef in (("sum", 1.25), ("mean", 0.0)):
            out = aggregate(h, b, mode, coef)
            outs += [out, torch.autograd.grad(out, h, torch.ones_like(out) * 0.5)[0]]
        pooled = hip_segment_mean(h, b.node_ptr, b.max_nodes)
        outs += [pooled, torch.autograd.grad(pooled, h, torch.ones_like(pooled) * 0.5)[0]]
        runs.append(outs)
    for a, c in zip(*runs):
        assert torch.equal(a, c)


# ---- twins against the restatement ---------------------------------------------------------------------------------
def _twin_inputs(eng, label="drnl", n_links=48, F=6):
    sp = _split("usair")
    li, _ = sp.all_links()
    x = torch.randn(sp.A.shape[0], F, generator=torch.Generator().manual_seed(9))
    subs = subgraphs(eng, li[:, ::97][:, :n_links], sp.A, 2, label, x=x)
    return subs, subs.batch(np.arange(len(subs))[::-1].copy())


def _ref_state(model):
    return {k: (v.detach().cpu().double().requires_grad_() if v.is_floating_point() else v.cpu())
            for k, v in model.state_dict().items()}


def _check_twin(model, b, forward, grad_keys, tol, training):
    """Logits and the gradients of `grad_keys` against the restatement `forward(sd, dtype)` in the same mode."""
    model.train(training)
    sd = _ref_state(model)                                # before the forward: BatchNorm's running stats move
    out = model(b)
    params = dict(model.named_parameters())
    grads = torch.autograd.grad(out.sum(), [params[k] for k in grad_keys])
    ref = forward(sd, torch.float64)
    ref_grads = torch.autograd.grad(ref.sum(), [sd[k] for k in grad_keys])
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=tol, atol=tol)
    for k, g, r in zip(grad_keys, grads, ref_grads):
        torch.testing.assert_close(g.cpu().double(), r, rtol=tol, atol=tol, msg=lambda m, k=k: f"{k}: {m}")


def _fp32_gap(forward, model):
    """max |restatement in fp32 - restatement in fp64| on these inputs: the size of fp32's own error here."""
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        return float((forward(sd, torch.float32).double() - forward(sd, torch.float64)).abs().max())


@pytest.mark.parametrize("training", [False, True])
def test_sage_twin_against_restatement(eng, training):
    from s3grl_amd.mpnn import SAGETwin

    torch.manual_seed(0)
    subs, b = _twin_inputs(eng)
    model = SAGETwin(32, 3, 1000, train_dataset=subs, use_feature=True, dropout=0.0).cuda()
    z, x, ei, ptr = b.z.cpu(), b.x.cpu(), b.edge_index.cpu(), b.node_ptr.cpu()

    def forward(sd, dtype):
        return sage_forward(sd, z, x, ei, ptr, num_convs=3, training=training, dtype=dtype)

    _check_twin(model, b, forward, [f"convs.{i}.lin_l.weight" for i in range(3)], 1e-4, training)


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("jk,train_eps", [(True, False), (False, False), (True, True)])
def test_gin_twin_against_restatement(eng, jk, train_eps, training):
    """GIN sums (not means) over USAir's dense subgraphs and normalises in every layer, so fp32's own error is larger
    than GCN's: the tolerance is the larger of GCNTwin's 1e-4 and 4 x the fp32-vs-fp64 gap of the RESTATEMENT on
    these inputs (never of the kernels' output)."""
    from s3grl_amd.mpnn import GINTwin

    torch.manual_seed(0)
    subs, b = _twin_inputs(eng)
    model = GINTwin(32, 3, 1000, train_dataset=subs, use_feature=True, jk=jk, train_eps=train_eps).cuda()
    model.mlp.dropout = 0.0
    if train_eps:
        with torch.no_grad():
            for c in [model.conv1] + list(model.convs):
                c.eps.fill_(0.25)
    z, x, ei, ptr = b.z.cpu(), b.x.cpu(), b.edge_index.cpu(), b.node_ptr.cpu()

    def forward(sd, dtype):
        return gin_forward(sd, z, x, ei, ptr, num_layers=3, jk=jk, training=training, dtype=dtype)

    gap = _fp32_gap(forward, model)
    tol = max(1e-4, 4 * gap)
    print(f"[mpnn] GIN jk={jk} train_eps={train_eps} training={training}: restatement fp32-fp64 gap {gap:.3e}, "
          f"tolerance {tol:.3e}")
    keys = ["conv1.nn.0.weight", "convs.0.nn.0.weight", "convs.1.nn.2.weight"]
    if train_eps:
        keys += ["conv1.eps", "convs.1.eps"]
    _check_twin(model, b, forward, keys, tol, training)


@pytest.mark.parametrize("with_x", [True, False])
@pytest.mark.parametrize("layer", ["GCN", "SAGE", "GIN"])
def test_net_twin_against_restatement(eng, layer, with_x):
    from s3grl_amd.mpgnn import NetTwin

    n, arcs = directed400()
    ei = torch.as_tensor(arcs.T.copy())
    x = torch.randn(n, 6, generator=torch.Generator().manual_seed(2)) if with_x else None
    net = NetTwin(6 if with_x else n, 32, layer, seed=5).cuda()
    graph = net.make_graph(ei, n)
    first = {"GCN": "lin.weight", "SAGE": "lin_l.weight", "GIN": "nn.0.weight"}[layer]
    keys = [f"conv{i}.{first}" for i in (1, 2, 3)]
    proj = torch.randn(n, 32, generator=torch.Generator().manual_seed(3))
    for training in (False, True):
        net.train(training)
        sd = _ref_state(net)
        z = net.encode(x.cuda() if with_x else None, graph, 0.0)
        params = dict(net.named_parameters())
        grads = torch.autograd.grad((z * proj.cuda()).sum(), [params[k] for k in keys])
        ref = net_forward(sd, x, ei, n, layer)
        ref_grads = torch.autograd.grad((ref * proj.double()).sum(), [sd[k] for k in keys])
        torch.testing.assert_close(z.detach().cpu().double(), ref.detach(), rtol=1e-4, atol=1e-4)
        for g, r in zip(grads, ref_grads):
            torch.testing.assert_close(g.cpu().double(), r, rtol=1e-4, atol=1e-4)
    logits = net.decode(z, ei.cuda())
    torch.testing.assert_close(logits, (z[ei[0].cuda()] * z[ei[1].cuda()]).sum(-1), rtol=1e-5, atol=1e-5)


# ---- end to end ----------------------------------------------------------------------------------------------------
# Floors: the lowest test AUC over seeds 1, 2, 3 of the TORCH RESTATEMENT (mpnn_reference.torch_operators: index_add
# aggregation, scatter mean pool) trained by the same loop on the same device, minus 0.02 for seed spread.  They are
# measured once per module run, not written down in advance (tools/mpgnn_probe.py --thresholds prints
# both sides).
SEEDS = (1, 2, 3)
_floors = {}


def _floor(key, train_one):
    if key not in _floors:
        with torch_operators():
            aucs = [train_one(seed) for seed in SEEDS]
        _floors[key] = min(aucs) - 0.02
        print(f"[mpnn] {key}: torch restatement test AUC {['%.4f' % a for a in aucs]}, floor {_floors[key]:.4f}")
    return _floors[key]


@pytest.fixture(scope="module")
def usair_split():
    return _split("usair", seed=1)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("model", ["SAGE", "GIN"])
def test_run_mpgnn_usair_auc(eng, usair_split, model, seed):
    from s3grl_amd.mpgnn import run_mpgnn

    def train_one(sd):
        return run_mpgnn(usair_split, model, None, epochs=50, seed=sd)["AUC"][1]

    floor = _floor(("mpgnn", model), train_one)
    auc = train_one(seed)
    print(f"[mpnn] USAir MPGNN {model} (x = None), 50 epochs, seed {seed}: test AUC {auc:.4f}")
    assert auc > floor, (auc, floor)


@pytest.fixture(scope="module")
def usair_seal(eng, usair_split):
    sp = usair_split

    def prep(name):
        pos, neg = sp.links[name]
        li = np.concatenate([pos, neg], axis=1)
        y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
        return subgraphs(eng, li, sp.A, 2, "drnl"), y

    return prep("train"), prep("test")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("model", ["SAGE", "GIN"])
def test_seal_mpnn_usair_auc(usair_seal, model, seed):
    from s3grl_amd.harness import train_and_evaluate_seal_mpnn

    train, test = usair_seal

    def train_one(sd):
        return train_and_evaluate_seal_mpnn(train, test, model=model, hidden=32, num_layers=3, epochs=4, lr=1e-3,
                                            seed=sd)[0]

    floor = _floor(("seal", model), train_one)
    auc = train_one(seed)
    print(f"[mpnn] USAir 2-hop {model}/drnl, 4 epochs at lr 1e-3, seed {seed}: test AUC {auc:.4f}")
    assert auc > floor, (auc, floor)
