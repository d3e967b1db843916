"""The four subgraph operators on the MI355X at every compiled instance, size edge and alignment: neighbour aggregation
(raw and GCN, csrc/s3grl_propagate.hip), segment mean (s3grl_mpnn.hip), SortPool (s3grl_seal_nn.hip) and centre pool
(s3grl_pool.hip), each against its fp64 restatement under the bounds of tests/subgraph_op_cases.py, which also holds
the sweeps (test_subgraph_ops_host.py shows that they reach every instance).  err / bound is printed and must be <= 1;
SortPool and every alignment and repeat check ask for bit-equal results."""
import collections

import numpy as np
import pytest
import torch

import oracle
import subgraph_op_cases as cases
from seal_nn_reference import gcn_norm, sort_pool

pytestmark = pytest.mark.gpu

U = cases.U
_worst = collections.defaultdict(float)


def note(op, *ratios):
    """Keeps the worst err / bound of an operator and asserts it."""
    r = max(ratios)
    _worst[op] = max(_worst[op], r)
    assert r <= 1.0, (op, ratios)
    return r


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd.engine import Engine

    e = Engine("cuda:0")
    yield e
    e.close()
    for op, r in sorted(_worst.items()):
        print(f"[subgraph ops] {op}: worst error / bound {r:.3f}")


def _randn(shape, seed):
    return torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))


class _Whole:
    """A whole graph as both operators, with its fp64 GCN arcs."""

    def __init__(self, n, arcs):
        from s3grl_amd.mpnn import NbrGraph
        from s3grl_amd.propagate import GcnGraph

        self.n = n
        self.ei = torch.as_tensor(arcs.T.copy()).cuda()
        self.nbr, self.gcn = NbrGraph(self.ei, n), GcnGraph(self.ei, n)
        self.arcs64 = gcn_norm(self.ei, n)


_wholes = {}


def whole(key):
    """The small graph ("small"), the edgeless one ("edgeless") or the ring of exactly `key` nodes, built once."""
    if key not in _wholes:
        n, arcs = cases.small_graph() if key == "small" else cases.edgeless_graph() if key == "edgeless" else \
            cases.ring_graph(key)
        _wholes[key] = _Whole(n, arcs)
    return _wholes[key]


@pytest.fixture(scope="module")
def small_subs(eng):
    """The directed 1-hop enclosing subgraphs of 30 links of the small graph, with its integer weights."""
    from s3grl_amd.seal import enclosing_subgraphs

    subs = enclosing_subgraphs(cases.small_links(), cases.small_graph_csr(), None, 0, 1, "drnl", directed=True,
                               engine=eng)
    assert len(subs) == 30
    return subs


# ---- aggregation ---------------------------------------------------------------------------------------------------
def check_aggregate(op, edge_index, H, mode, self_coef, seed):
    from s3grl_amd.mpnn import aggregate

    n = op.num_nodes
    h = _randn((n, H), seed).requires_grad_()
    gout = _randn((n, H), seed + 1)
    out = aggregate(h, op, mode, self_coef)
    (gh,) = torch.autograd.grad(out, h, gout)
    ref, bound, ref_g, bound_g = cases.aggregate_reference(h.detach().double(), gout.double(), edge_index[0],
                                                           edge_index[1], mode, self_coef)
    return note("raw aggregation", cases.ratio(out.detach(), ref, bound), cases.ratio(gh, ref_g, bound_g))


def check_gcn(call, n, arcs64, H, with_bias, seed):
    """call(h, bias) -> out; arcs64 = gcn_norm(...) of the same operator in fp64."""
    h = _randn((n, H), seed).requires_grad_()
    bias = _randn((H,), seed + 1).requires_grad_() if with_bias else None
    gout = _randn((n, H), seed + 2)
    out = call(h, bias)
    grads = torch.autograd.grad(out, (h, bias) if with_bias else (h,), gout)
    ref, bound, ref_g, bound_g = cases.gcn_reference(h.detach().double(), gout.double(),
                                                     bias.detach().double() if with_bias else None, *arcs64)
    if with_bias:
        torch.testing.assert_close(grads[1], gout.sum(0))            # torch's own sum, as gcn_propagate returns it
    return note("GCN propagation", cases.ratio(out.detach(), ref, bound), cases.ratio(grads[0], ref_g, bound_g))


@pytest.mark.parametrize("H", cases.AGG_H)
def test_aggregation_on_the_whole_small_graph(eng, H):
    g = whole("small")
    worst = 0.0
    for mode in ("sum", "mean"):
        for self_coef in (0.0, 1.25):
            worst = max(worst, check_aggregate(g.nbr, g.ei, H, mode, self_coef, seed=H))
    for with_bias in (True, False):
        worst = max(worst, check_gcn(g.gcn.propagate, g.n, g.arcs64, H, with_bias, seed=3 * H))
    print(f"[subgraph ops] whole graph, H = {H} {cases.agg_path(H)}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("H", cases.AGG_H)
def test_aggregation_on_subgraph_batches(small_subs, H):
    from s3grl_amd.seal_nn import gcn_propagate

    subs = small_subs
    worst = 0.0
    for ids in (np.arange(30), np.random.default_rng(5).permutation(30)[:17]):
        for use_w in (True, False):
            b = subs.batch(ids, use_edge_weight=use_w)
            assert (ids.size == 30) == bool(torch.equal(b.rows, torch.arange(b.num_nodes, device="cuda")))
            ei = b.edge_index
            arcs64 = gcn_norm(ei, b.num_nodes, b.edge_weight if use_w else None)
            if use_w:
                assert int(b.edge_weight.max()) > 1
            worst = max(worst, check_gcn(lambda h, bias, b=b: gcn_propagate(h, b, bias), b.num_nodes, arcs64, H, True,
                                         seed=5 * H))
        for mode in ("sum", "mean"):
            for self_coef in (0.0, 1.25):
                worst = max(worst, check_aggregate(b, ei, H, mode, self_coef, seed=7 * H))
    print(f"[subgraph ops] subgraph batches, H = {H} {cases.agg_path(H)}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("H", [1, 2, 3, 5, 9, 17, 33, 4, 8, 12, 20, 36, 68, 132])
def test_aggregation_row_count_edges(eng, H):
    """Whole graphs of exactly 1, per_block - 1, per_block and per_block + 1 nodes, for one H of every (VEC, LPN)."""
    per_block = cases.agg_rows_per_block(H)
    assert per_block == 4 * 64 // cases.agg_path(H)[1]
    worst = 0.0
    for n in sorted({1, per_block - 1, per_block, per_block + 1}):
        g = whole(n)
        assert g.nbr.num_nodes == n and g.gcn.num_nodes == n
        worst = max(worst, check_aggregate(g.nbr, g.ei, H, "sum", 1.25, seed=n + H),
                    check_aggregate(g.nbr, g.ei, H, "mean", 0.0, seed=n + H),
                    check_gcn(g.gcn.propagate, n, g.arcs64, H, True, seed=n + 2 * H))
    print(f"[subgraph ops] row-count edges, H = {H}, per_block = {per_block}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("H", [1, 5, 36, 260])
def test_aggregation_on_the_edgeless_graph(eng, H):
    from s3grl_amd.mpnn import aggregate

    g = whole("edgeless")
    assert g.nbr.in_nbr.numel() == 0
    h = _randn((g.n, H), H).requires_grad_()
    gout = _randn((g.n, H), H + 1)
    for self_coef, want, want_g in ((0.0, torch.zeros_like(h), torch.zeros_like(h)), (1.0, h.detach(), gout),
                                    (1.25, h.detach() * 1.25, gout * 1.25)):
        for mode in ("sum", "mean"):                                # no arc: the mean is a zero row, never NaN
            out = aggregate(h, g.nbr, mode, self_coef)
            (gh,) = torch.autograd.grad(out, h, gout)
            assert torch.equal(out.detach(), want) and torch.equal(gh, want_g), (mode, self_coef)
    bias = _randn((H,), H + 2)
    out = g.gcn.propagate(h, bias)                                  # one loop per node, dinv = 1: h + bias
    (gh,) = torch.autograd.grad(out, h, gout)
    assert torch.equal(out.detach(), h.detach() + bias) and torch.equal(gh, gout)
    assert torch.equal(g.gcn.propagate(h).detach(), h.detach())
    check_gcn(g.gcn.propagate, g.n, g.arcs64, H, True, seed=H)


def test_gcn_norm_with_an_empty_row_and_weights(eng):
    from s3grl_amd import _native as N

    ptr = torch.tensor([0, 2, 2, 5, 5, 6], dtype=torch.int64, device="cuda")
    w = torch.tensor([1.0, 3.0, 2.0, 2.0, 4.0, 3.0], device="cuda")
    for weight, deg in ((w, [4.0, 0.0, 8.0, 0.0, 3.0]), (None, [2.0, 0.0, 3.0, 0.0, 1.0])):
        dinv = torch.full((5,), float("nan"), device="cuda")
        N.check(N.lib().s3grl_gcn_norm(eng._ctx, 5, N.ptr(ptr), N.ptr(weight), N.ptr(dinv)), "s3grl_gcn_norm")
        ref = torch.tensor(deg, dtype=torch.float64, device="cuda").pow(-0.5)
        ref[torch.isinf(ref)] = 0.0
        assert float(dinv[1]) == 0.0 and float(dinv[3]) == 0.0       # an empty row: 0, not inf
        note("gcn_norm", cases.ratio(dinv, ref, 4 * U * ref))        # sqrtf and the reciprocal, 2u each


# ---- segment mean --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", cases.SEG_W)
def test_segment_mean_every_instance(eng, W):
    from s3grl_amd.mpnn import segment_mean as hip_segment_mean

    full = cases.segments(cases.SEG_SIZES)
    prefix = full[:cases.SEG_PREFIX + 1]                            # no graph longer than a chunk: chunks == 1
    x_all = _randn((int(full[-1]), W), W)
    worst = 0.0
    for ptr in (full, prefix):
        sizes = ptr.diff()
        pd = ptr.cuda()
        xs = x_all[:int(ptr[-1])].detach().requires_grad_()
        gout = _randn((sizes.numel(), W), W + 1)
        ref, bound, ref_g, bound_g = cases.segment_mean_reference(xs.detach().double(), gout.double(), pd)
        for max_nodes in (int(sizes.max()), None):
            out = hip_segment_mean(xs, pd, max_nodes)
            (gx,) = torch.autograd.grad(out, xs, gout)
            worst = max(worst, note("segment mean", cases.ratio(out.detach(), ref, bound),
                                    cases.ratio(gx, ref_g, bound_g)))
            assert bool((out[sizes.cuda() == 0] == 0).all())         # an empty graph: a zero row
    print(f"[subgraph ops] segment mean W = {W} {cases.seg_path(W)}: worst error / bound {worst:.3f}")


# ---- SortPool --------------------------------------------------------------------------------------------------
def pool_case(sizes, D, seed, keys=None):
    g = torch.Generator().manual_seed(seed)
    n = int(sum(sizes))
    x = torch.randn((n, D), generator=g)
    if keys is not None:
        x[:, -1] = keys(n, g)
    return x, cases.segments(sizes)


def three_values(n, g):
    return torch.randint(0, 3, (n,), generator=g).float() * 0.5


def run_sort_pool(x, ptr, k, lds_budget=0, gout=None):
    from s3grl_amd.seal_nn import sort_pool as hip_sort_pool

    xd = x.cuda().requires_grad_()
    out, index = hip_sort_pool(xd, ptr.cuda(), k, int(ptr.diff().max()), lds_budget, return_index=True)
    if gout is None:
        gout = _randn(out.shape, 1)
    (gx,) = torch.autograd.grad(out, xd, gout)
    return out.detach(), index, gx, gout


def check_sort_pool(x, ptr, k, lds_budget=0):
    """out, index and grad_x equal the restatement's exactly."""
    out, index, gx, gout = run_sort_pool(x, ptr, k, lds_budget)
    ref, ref_index = sort_pool(x.double(), ptr, k)
    assert torch.equal(index.cpu().long(), ref_index)
    assert torch.equal(out.cpu(), ref.float())
    xr = x.double().requires_grad_()
    (ref_gx,) = torch.autograd.grad(sort_pool(xr, ptr, k, ref_index)[0], xr, gout.cpu().double())
    assert torch.equal(gx.cpu(), ref_gx.float())
    return out, index, gx, gout


@pytest.mark.parametrize("D", cases.COPY_D)
def test_sort_pool_every_width(eng, D):
    x, ptr = pool_case([3, 12, 0, 40, 1, 13], D, D)                 # n < k, n = k, an empty graph inside, n > k
    for k in (1, 12):
        _, index, _, _ = check_sort_pool(x, ptr, k)
        assert bool((index[2] == -1).all())
        check_sort_pool(x, ptr, k, lds_budget=1)                   # every graph through the HBM sort


@pytest.mark.parametrize("keys", [None, three_values], ids=["random", "three_values"])
@pytest.mark.parametrize("D", [4, 97])
def test_sort_pool_sizes_past_one_trip_of_the_sort(eng, D, keys):
    """257 .. 8193 nodes: P = 512 .. 16384, so the compare-exchange loop takes 1, 2, 4, 16 and 32 trips; 8192 keys
    are the last that fit the default LDS budget, 8193 nodes sort in HBM.  At D = 4 k is the longest graph, so the
    whole order is compared; three-valued keys leave the order to the position tie-break."""
    sizes = [5, 257, 513, 0, 1025, 8192, 8193, 12]
    x, ptr = pool_case(sizes, D, 10 + D, keys)
    k = 8193 if D == 4 else 300
    hbm = check_sort_pool(x, ptr, k)                               # the default budget: 8193 nodes in HBM
    lds = run_sort_pool(x, ptr, k, lds_budget=159 << 10, gout=hbm[3])   # the declared maximum: 16384 keys in LDS
    for a, b in zip(hbm[:3], lds[:3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("D", [4, 97])
def test_sort_pool_1025_nodes_in_hbm_equal_lds(eng, D):
    x, ptr = pool_case([5, 1025, 3], D, 20 + D, three_values)
    lds = check_sort_pool(x, ptr, 1025)
    hbm = run_sort_pool(x, ptr, 1025, lds_budget=1, gout=lds[3])
    for a, b in zip(lds[:3], hbm[:3]):
        assert torch.equal(a, b)


# ---- centre pool -----------------------------------------------------------------------------------------------
POOL_COUNTS = [2, 5, 2, 3, 9, 2, 4, 2, 7, 3, 2]                     # 11 links: three workgroups, the last not full


@pytest.mark.parametrize("mode", ["", "mean", "sum"])
@pytest.mark.parametrize("H", cases.POOL_H)
def test_centre_pool_every_width_and_mode(eng, H, mode):
    from s3grl_amd.pool import centre_pool

    rp = cases.segments(POOL_COUNTS)
    h = _randn((int(rp[-1]), H), H).requires_grad_()
    k = 1 if mode else 0
    out = centre_pool(h, rp.cuda(), k_heuristic=k, k_pool_strategy=mode)
    hd = h.detach().double()
    ref = oracle.centre_pool(hd.cpu().numpy(), rp.numpy(), k_heuristic=k, k_pool_strategy=mode)
    assert out.shape == ref.shape
    fwd = cases.ratio(out.detach(), torch.as_tensor(ref).cuda(), cases.centre_pool_bound(hd, rp, mode))
    gout = _randn(out.shape, H + 1)
    h2 = hd.clone().requires_grad_()
    (ref_g,) = torch.autograd.grad(cases.centre_pool_torch(h2, rp, mode), h2, gout.double())
    poison = torch.full_like(h, float("nan"))                      # grad_h is torch.empty_like(h): a row the backward
    del poison                                                     # skipped would likely show this block, not a zero
    (gh,) = torch.autograd.grad(out, h, gout)
    further = torch.ones(h.shape[0], dtype=torch.bool)
    further[rp[:-1]] = False
    further[rp[:-1] + 1] = False
    assert int(further.sum()) == sum(POOL_COUNTS) - 2 * len(POOL_COUNTS)
    if not mode:
        assert bool((gh[further.cuda()] == 0).all())               # rows past the second: exact zeros
    bwd = cases.ratio(gh, ref_g, 2 * U * ref_g.abs())
    r = note("centre pool", fwd, bwd)
    print(f"[subgraph ops] centre pool H = {H} {cases.copy_path(H, 'centre')} {mode or 'none'}: "
          f"worst error / bound {r:.3f}")


# ---- misaligned inputs -----------------------------------------------------------------------------------------
def _misaligned(t):
    """t's values in a contiguous tensor that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _both_layouts(monkeypatch, call, inputs, gout, expect_copies):
    """call(*leaves) -> out, run on aligned inputs and on misaligned ones (the upstream gradient too): outputs and
    gradients bit-equal, and the wrapper's aligned16 saw exactly `expect_copies` misaligned tensors."""
    from s3grl_amd import _native

    seen = []
    orig = _native.aligned16

    def spy(t):
        seen.append(t.data_ptr() % 16)
        return orig(t)

    monkeypatch.setattr(_native, "aligned16", spy)
    results = []
    for layout in (lambda t: t.clone(), _misaligned):
        del seen[:]
        leaves = [layout(t).detach().requires_grad_() for t in inputs]
        w = layout(gout)
        mis = layout is _misaligned
        for t in leaves + [w]:
            assert t.is_contiguous() and (t.data_ptr() % 16 == 4) == mis
        out = call(*leaves)
        grads_seen = []
        out.register_hook(lambda g, grads_seen=grads_seen: grads_seen.append(g.data_ptr() % 16))
        out.backward(w)
        assert grads_seen == [4 if mis else 0]                      # the gradient reached the backward as it was
        assert sum(1 for a in seen if a) == (expect_copies if mis else 0), seen
        results.append([out.detach()] + [t.grad for t in leaves])
    for a, b in zip(*results):
        assert a is not None and torch.equal(a, b)


def test_misaligned_gcn_propagate(small_subs, monkeypatch):
    from s3grl_amd.propagate import GicGraph
    from s3grl_amd.seal_nn import gcn_propagate

    g = whole("small")
    gic = GicGraph(g.ei, g.n)
    b = small_subs.batch(np.arange(30), use_edge_weight=True)
    for n, call in ((g.n, g.gcn.propagate), (g.n, gic.propagate),
                    (b.num_nodes, lambda h, bias: gcn_propagate(h, b, bias))):
        _both_layouts(monkeypatch, call, [_randn((n, 36), 1), _randn((36,), 2)], _randn((n, 36), 3), 3)


def test_misaligned_aggregate(eng, monkeypatch):
    from s3grl_amd.mpnn import aggregate

    g = whole("small")
    _both_layouts(monkeypatch, lambda h: aggregate(h, g.nbr, "mean", 1.25), [_randn((g.n, 36), 4)],
                  _randn((g.n, 36), 5), 2)


def test_misaligned_sort_pool(eng, monkeypatch):
    from s3grl_amd.seal_nn import sort_pool as hip_sort_pool

    x, ptr = pool_case([3, 12, 0, 40, 1, 13], 8, 6)
    pd = ptr.cuda()
    _both_layouts(monkeypatch, lambda x: hip_sort_pool(x, pd, 12, 40), [x.cuda()], _randn((6, 12 * 8), 7), 2)


def test_misaligned_centre_pool(eng, monkeypatch):
    from s3grl_amd.pool import centre_pool

    rp = cases.segments(POOL_COUNTS).cuda()
    n = sum(POOL_COUNTS)
    for mode in ("", "mean"):
        _both_layouts(monkeypatch, lambda h: centre_pool(h, rp, 1 if mode else 0, mode), [_randn((n, 8), 8)],
                      _randn((len(POOL_COUNTS), 16 if mode else 8), 9), 2)


# ---- determinism -----------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(small_subs):
    from s3grl_amd.mpnn import aggregate
    from s3grl_amd.mpnn import segment_mean as hip_segment_mean
    from s3grl_amd.pool import centre_pool
    from s3grl_amd.seal_nn import gcn_propagate
    from s3grl_amd.seal_nn import sort_pool as hip_sort_pool

    b = small_subs.batch(np.arange(30), use_edge_weight=True)
    seg = cases.segments(cases.SEG_SIZES).cuda()
    xp, pp = pool_case([5, 1025, 0, 300], 8, 3, three_values)
    rp = cases.segments(POOL_COUNTS).cuda()
    runs = []
    for _ in range(2):
        outs = []

        def both(fn, x):
            x = x.detach().requires_grad_()
            out = fn(x)
            outs.extend([out.detach(), torch.autograd.grad(out, x, torch.full_like(out, 0.5))[0]])

        bias = _randn((65,), 2)
        both(lambda h: gcn_propagate(h, b, bias), _randn((b.num_nodes, 65), 1))
        both(lambda h: aggregate(h, b, "mean", 1.25), _randn((b.num_nodes, 68), 3))
        both(lambda x: hip_segment_mean(x, seg, max(cases.SEG_SIZES)), _randn((int(seg[-1]), 33), 4))
        both(lambda x: hip_sort_pool(x, pp.cuda(), 400, 1025), xp.cuda())
        both(lambda h: centre_pool(h, rp, 1, "mean"), _randn((sum(POOL_COUNTS), 260), 5))
        runs.append(outs)
    assert len(runs[0]) == 10
    for a, c in zip(*runs):
        assert torch.equal(a, c)
