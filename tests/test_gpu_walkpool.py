"""WalkPool on the MI355X against the dense restatement (tests/walkpool_reference.py): the two operators forward and
backward, their LDS / HBM flavours, the model twin teacher-forced through three Adam steps, and run_walkpool.

Bounds.  Attention: every weight within (8 + deg_in + 4)·2^-23 relative to its fp64 value — rounding
the shifted exponent (|w - max| <= 16: 8 units of 2^-23), the deg_in-term sum, and exp with the division.  The bound
has no term for the dot product, so q and k are drawn as multiples of 1/4 whose products and sums are exact in fp32;
the one rounding of the division by sqrt(hidden) is inside the 8.  Walk profile: tau·(d_max + 2)·2^-23·M, all terms
being non-negative with one rounding per product and per sum term over tau pulls; M is the feature's own magnitude,
tr(X+) + tr(X-) for graphlevel.  Gradients and the trained model: the error of the restatement itself in fp32 on the
CPU is the yardstick; the GPU may be at most 8 times off it (the summation orders differ), with a floor of 2^-20.

Bit equality by construction: an element of X never depends on the column block or the flavour, so nodelevel and
linklevel are bit-identical between every lds_budget and between a batch and its links one at a time; with one column
block and group count (lds_budget = 1 against the budget that forces W = 4 in LDS) graphlevel and both gradients are
bit-identical as well."""
import math

import numpy as np
import pytest
import torch

import walkpool_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -23
FLOOR = 2.0 ** -20


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd.engine import Engine

    e = Engine("cuda:0")
    yield e
    e.close()


# ---- lists ---------------------------------------------------------------------------------------------------------
def _random_graph(n, rng, extra=1.0):
    """Connected, no edge between 0 and 1: node v >= 2 hangs on an earlier node, then n·extra random edges."""
    edges = set()
    for v in range(2, n):
        u = int(rng.integers(0, v))
        edges.add((u, v))
    for _ in range(int(n * extra)):
        u, v = sorted(int(t) for t in rng.integers(0, n, 2))
        if u != v and (u, v) != (0, 1):
            edges.add((u, v))
    return n, sorted(edges)


HAND_SIZES = (3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)


def _hand_graphs():
    rng = np.random.default_rng(7)
    graphs = [(2, []),                                        # 0: an isolated pair
              (3, [(0, 2), (1, 2)]),                          # 1: the triangle
              (3, [(0, 2)]),                                  # 2: node 1's only neighbour is node 0
              (10, [(0, c) for c in range(2, 10)])]           # 3: a star around node 0, node 1 a leaf by the link alone
    graphs += [_random_graph(n, rng) for n in HAND_SIZES]
    return graphs


def _make_list(graphs, dev, x_width=4):
    """A SubgraphList of hand-made subgraphs (n, undirected edges without (0, 1))."""
    from s3grl_amd.seal import LabelledSubgraphs, SubgraphList

    node_ptr, edge_ptr, src, dst = [0], [0], [], []
    for n, edges in graphs:
        node_ptr.append(node_ptr[-1] + n)
        src += [a for a, b in edges] + [b for a, b in edges]
        dst += [b for a, b in edges] + [a for a, b in edges]
        edge_ptr.append(len(src))
    total = node_ptr[-1]
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)   # noqa: E731
    subs = LabelledSubgraphs(node_ptr=t(node_ptr, torch.int64), nodes=torch.arange(total, dtype=torch.int32, device=dev),
                             dists=torch.zeros(total, dtype=torch.int8, device=dev), edge_ptr=t(edge_ptr, torch.int64),
                             src=t(src, torch.int32), dst=t(dst, torch.int32),
                             weight=torch.ones(len(src), dtype=torch.float32, device=dev),
                             z=torch.zeros(total, dtype=torch.int32, device=dev))
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(total, x_width, generator=gen).to(dev)
    return SubgraphList(subs, x, 0, torch.float32, "zo")


def _graphs_of(subs):
    """[(n, src, dst)] of a SubgraphList on the host, for the restatement."""
    s = subs.subs
    src, dst = s.src.cpu().long(), s.dst.cpu().long()
    out = []
    for g in range(len(subs)):
        a, b = subs._edge_ptr[g], subs._edge_ptr[g + 1]
        out.append((subs._node_ptr[g + 1] - subs._node_ptr[g], src[a:b], dst[a:b]))
    return out


def _topology(name):
    from conftest import csr_from_undirected, load_extract
    from s3grl_amd import workloads as W

    if name == "usair":
        n, e = W.load_topology("usair")
    else:
        g = load_extract(name)
        n, e = int(g["num_nodes"]), g["edges"]
    e = np.asarray(e, dtype=np.int64)
    return n, e, csr_from_undirected(n, e)


@pytest.fixture(scope="module")
def lists(eng):
    """name -> (WalkPoolSplit, graphs): the hand-made list and a few links of rand300 and usair at 1 and 2 hops
    (positives, whose link leaves the subgraph, and negatives)."""
    from s3grl_amd.seal import enclosing_subgraphs
    from s3grl_amd.walkpool import WalkPoolSplit

    out = {}
    hand = _make_list(_hand_graphs(), eng.device)
    out["hand"] = (WalkPoolSplit(hand), _graphs_of(hand))
    for name, hops, count in (("rand300", 1, 4), ("rand300", 2, 3), ("usair", 1, 4), ("usair", 2, 2)):
        n, e, A = _topology(name)
        rng = np.random.default_rng(11)
        pos = e[rng.choice(len(e), count // 2, replace=False)]
        neg = np.array([[5, 77], [120, 9]])[:count - count // 2]
        li = np.concatenate([pos, neg]).T
        x = torch.ones((n, 4), dtype=torch.float32)
        subs = enclosing_subgraphs(li, A, x, 0, hops, "zo", engine=eng)
        out[f"{name}_h{hops}"] = (WalkPoolSplit(subs), _graphs_of(subs))
    return out


def _dyadic(shape, hidden, seed, dev):
    """Multiples of 1/4 with |w| <= 8 after the division by sqrt(hidden): products and sums exact in fp32."""
    lim = 4 if hidden >= 32 else 6                            # |q|, |k| <= 1 or 1.5
    gen = torch.Generator().manual_seed(seed)
    t = torch.randint(-lim, lim + 1, shape, generator=gen).to(torch.float32) / 4
    assert hidden * (lim / 4) ** 2 / math.sqrt(hidden) <= 8
    return t.to(dev)


def _arcs(batch):
    """Host (link, local src, local dst, mask) of every batch arc in the kernels' in-order, and deg_in per arc."""
    ei, mask = batch.in_edge_index()
    link = batch.link.long()[ei[1]]
    first = batch.node_ptr[:-1][link]
    deg = batch.in_ptr.diff()[ei[1]]
    return link.cpu(), (ei[0] - first).cpu(), (ei[1] - first).cpu(), mask.cpu(), deg.cpu()


def _small_budget(batch):
    return 2 * max(batch.max_nodes, 2) * 4 * 4                # the forward's ping-pong at W = 4 and nothing wider


# ---- structure -----------------------------------------------------------------------------------------------------
def test_split_arc_bookkeeping(eng):
    from s3grl_amd.walkpool import WalkPoolSplit

    subs = _make_list([(3, [(0, 2), (1, 2)]), (4, [(0, 2), (2, 3), (1, 3)])], eng.device)
    wps = WalkPoolSplit(subs)
    assert wps.arc_ptr.tolist() == [0, 6, 14] and wps.num_arcs == 14
    assert subs._gcn == {} and subs._nbr is None              # the SubgraphList is not changed
    for ids in ([0, 1], [1], [1, 0]):
        b = wps.batch(ids)
        link, s, d, mask, deg = _arcs(b)
        assert b.num_arcs == sum(6 if i == 0 else 8 for i in ids) and b.max_arcs == max(6 if i == 0 else 8 for i in ids)
        for pos, i in enumerate(ids):
            sel = link == pos
            edges = [(0, 2), (1, 2)] if i == 0 else [(0, 2), (2, 3), (1, 3)]
            want = sorted([(a, c) for a, c in edges] + [(c, a) for a, c in edges] + [(0, 1), (1, 0)],
                          key=lambda p: (p[1], p[0]))
            assert list(zip(s[sel].tolist(), d[sel].tolist())) == want          # by target, then by source
            cand = [(a, c) for a, c, m in zip(s[sel].tolist(), d[sel].tolist(), mask[sel].tolist()) if not m]
            assert cand == [(1, 0), (0, 1)]
        assert torch.equal(b.in_dst.cpu().long(), d)
        # the out-order names the same arcs
        out_src = torch.repeat_interleave(torch.arange(b.num_nodes), b.out_ptr.diff().cpu())
        first = b.node_ptr[:-1].cpu()[b.link.long().cpu()]
        oa = b.out_arc.cpu()
        assert torch.equal(s[oa] + first[out_src], out_src)
        assert torch.equal(d[oa], b.out_nbr.cpu().long())
        assert sorted(oa.tolist()) == list(range(b.num_arcs))
        # the GCN operator is that of E+: degree + 1 self-loop
        dinv = b.gcn.dinv[b.rows].cpu()
        indeg = b.in_ptr.diff().cpu().float()
        assert torch.allclose(dinv, (indeg + 1).pow(-0.5))


def test_errors(eng):
    from s3grl_amd.seal import enclosing_subgraphs
    from s3grl_amd.walkpool import WalkPoolSplit, walk_pool

    n, e, A = _topology("usair")
    with pytest.raises(ValueError, match="src == dst"):
        enclosing_subgraphs(np.array([[3], [3]]), A, None, 0, 1, "zo", engine=eng)
    with pytest.raises(ValueError, match="outside"):
        enclosing_subgraphs(np.array([[3], [n]]), A, None, 0, 1, "zo", engine=eng)
    with pytest.raises(ValueError, match="must not contain the link"):
        WalkPoolSplit(_make_list([(3, [(0, 1), (1, 2)])], eng.device))
    big = WalkPoolSplit(_make_list([(4097, [(v, v + 1) for v in range(1, 4096)] + [(0, 4096)])], eng.device))
    b = big.batch([0])
    w = torch.zeros((b.num_arcs, 1), device=eng.device)
    with pytest.raises(NotImplementedError, match="4096"):
        walk_pool(w, w, b, 2)
    with pytest.raises(ValueError, match="walk_len"):
        walk_pool(w, w, b, 17)


# ---- attention -----------------------------------------------------------------------------------------------------
def _attention_reference(graphs, q, k, dtype):
    """Per link (P+, P-, omega) of the restatement in `dtype`; q, k host tensors over the batch's nodes."""
    out, a = [], 0
    for n, src, dst in graphs:
        out.append(R.attention_dense(q[a:a + n].to(dtype), k[a:a + n].to(dtype), n, src, dst)[:3])
        a += n
    return out


@pytest.mark.parametrize("hidden", [8, 32])
@pytest.mark.parametrize("heads", [1, 2, 3])
def test_attention_forward(eng, lists, heads, hidden):
    from s3grl_amd.walkpool import attention_weights

    worst = 0.0
    for name, (wps, graphs) in lists.items():
        b = wps.batch(np.arange(len(wps)))
        q = _dyadic((b.num_nodes, heads, hidden), hidden, 1, eng.device)
        k = _dyadic((b.num_nodes, heads, hidden), hidden, 2, eng.device)
        wp, wm, om = attention_weights(q, k, b)
        wp2, wm2, om2 = attention_weights(q, k, b)
        assert torch.equal(wp, wp2) and torch.equal(wm, wm2) and torch.equal(om, om2)
        ref = _attention_reference(graphs, q.cpu(), k.cpu(), torch.float64)
        link, s, d, mask, deg = _arcs(b)
        ref_p = torch.stack([ref[g][0][:, c, r] for g, r, c in zip(link.tolist(), s.tolist(), d.tolist())])
        ref_m = torch.stack([ref[g][1][:, c, r] for g, r, c in zip(link.tolist(), s.tolist(), d.tolist())])
        ref_o = torch.stack([r[2] for r in ref])
        bound = ((8 + deg + 4) * U).double()[:, None]
        err_p = ((wp.cpu().double() - ref_p).abs() / ref_p / bound).max().item()
        live = ref_m > 0
        err_m = (((wm.cpu().double() - ref_m).abs() / ref_m.clamp(min=1e-300) / bound)[live]).max().item() \
            if live.any() else 0.0
        err_o = ((om.cpu().double() - ref_o).abs() / ((8 + 4) * U)).max().item()
        print(f"attention {name} heads {heads} hidden {hidden}: error / bound p {err_p:.3f} m {err_m:.3f} "
              f"omega {err_o:.3f}")
        assert bool((wm.cpu()[~mask] == 0).all()) and bool((ref_m[~mask] == 0).all())
        assert bool((wm.cpu()[~live] == 0).all())             # a node whose only in-arc is the candidate
        worst = max(worst, err_p, err_m, err_o)
    assert worst <= 1.0


# ---- walk profile --------------------------------------------------------------------------------------------------
def _gpu_weights(eng, b, heads, seed=5):
    from s3grl_amd.walkpool import attention_weights

    gen = torch.Generator().manual_seed(seed)
    q = torch.randn((b.num_nodes, heads, 8), generator=gen).to(eng.device)
    k = torch.randn((b.num_nodes, heads, 8), generator=gen).to(eng.device)
    wp, wm, _ = attention_weights(q, k, b)
    return wp, wm


def _dense_weights(graphs, arcs, w, dtype):
    """Per link the dense [heads, n, n] of per-arc weights w (host, the batch's in-order)."""
    link, s, d = arcs[:3]
    return [R.weights_to_dense(w[link == g].to(dtype), n, s[link == g], d[link == g])
            for g, (n, _, _) in enumerate(graphs)]


@pytest.fixture(scope="module")
def walk_cases(eng, lists):
    """(name, heads) -> (batch, weights_p, weights_m, fp64 features [B, heads, 7, 5], traces [B, heads, 7, 2], d_max
    [B]): the restatement on the fp32 weights the GPU made, computed once for walk_len 7 (shorter walks are a prefix)."""
    cache = {}

    def get(name, heads):
        if (name, heads) not in cache:
            wps, graphs = lists[name]
            b = wps.batch(np.arange(len(wps)))
            wp, wm = _gpu_weights(eng, b, heads)
            arcs = _arcs(b)
            Pp = _dense_weights(graphs, arcs, wp.cpu(), torch.float64)
            Pm = _dense_weights(graphs, arcs, wm.cpu(), torch.float64)
            both = [R.walk_features(p, m, 7) for p, m in zip(Pp, Pm)]
            dmax = torch.tensor([int(arcs[4][arcs[0] == g].max()) for g in range(len(graphs))], dtype=torch.float64)
            cache[name, heads] = (b, wp, wm, torch.stack([f for f, _ in both]), torch.stack([t for _, t in both]), dmax)
        return cache[name, heads]

    return get


def _walk_bound(feat, traces, dmax, walk_len):
    """[B, heads, walk_len, 5]: tau·(d_max + 2)·2^-23·M."""
    M = feat[:, :, :walk_len].abs().clone()
    M[..., 0] = traces[:, :, :walk_len].sum(-1)
    tau = torch.arange(2, walk_len + 2, dtype=torch.float64)[None, None, :, None]
    return tau * (dmax[:, None, None, None] + 2) * U * M


@pytest.mark.parametrize("heads", [1, 2, 3])
def test_walk_forward(eng, lists, walk_cases, heads):
    from s3grl_amd.walkpool import walk_pool

    worst = 0.0
    for name in lists:
        b, wp, wm, feat, traces, dmax = walk_cases(name, heads)
        for walk_len in (1, 2, 7):
            bound = _walk_bound(feat, traces, dmax, walk_len)
            outs = {}
            for lds in (0, _small_budget(b), 1):
                out = walk_pool(wp, wm, b, walk_len, lds_budget=lds)
                assert torch.equal(out, walk_pool(wp, wm, b, walk_len, lds_budget=lds))       # two runs
                err = (out.cpu().double() - feat[:, :, :walk_len]).abs()
                ratio = (err / bound.clamp(min=1e-300))[bound > 0].max().item()
                assert bool((err[bound == 0] == 0).all())
                worst = max(worst, ratio)
                outs[lds] = out
            print(f"walk {name} heads {heads} walk_len {walk_len}: error / bound {worst:.3f}")
            a, c, h = outs[0], outs[_small_budget(b)], outs[1]
            assert torch.equal(c, h)                          # W = 4 and the same groups, LDS against HBM
            assert torch.equal(a[..., 1:], c[..., 1:])        # elements of X do not depend on the block
            assert bool(((a[..., 0] - c[..., 0]).abs().cpu().double() <= bound[..., 0]).all())
    assert worst <= 1.0


def test_walk_known_answers_and_batch_against_single_links(eng, lists, walk_cases):
    from s3grl_amd.walkpool import attention_weights, walk_pool

    wps, graphs = lists["hand"]
    # all logits 0 on the pair and the triangle: the hand-derived answers, exact in fp32 but for the thirds
    b = wps.batch([0, 1])
    z = torch.zeros((b.num_nodes, 1, 8), device=eng.device)
    wp, wm, om = attention_weights(z, z, b)
    out = walk_pool(wp, wm, b, 4).cpu()[:, 0]
    assert om.cpu().tolist() == [[1.0], [1.0]]
    assert out[0, :, 0].tolist() == [2, 0, 2, 0] and out[0, :, 1].tolist() == [2, 0, 2, 0]
    assert out[0, :, 3].tolist() == [0, 2, 0, 2] and out[0, :, 2].abs().sum() == 0 and out[0, :, 4].abs().sum() == 0
    for t, tau in enumerate((2, 3, 4, 5)):
        a, even = (-0.5) ** tau, float(tau % 2 == 0)
        want = [(1 + 2 * a) - 2 * even, 2 * (1 + 2 * a) / 3, even, 2 * (1 - a) / 3, even]
        assert out[1, t].tolist() == pytest.approx(want, abs=8 * U)
    # one batch that mixes n = 2 with the largest subgraph, against its links one at a time
    for name, heads in (("hand", 2), ("usair_h2", 2)):
        wps, graphs = lists[name]
        bfull, wp, wm, feat, traces, dmax = walk_cases(name, heads)
        big = int(np.argmax(wps.subs.node_counts()))
        ids = [0, big] if name == "hand" else [big, 0]
        arc_ptr = np.concatenate([[0], np.cumsum(np.diff(wps.arc_ptr))])
        mixed = wps.batch(ids)
        sel = torch.cat([torch.arange(arc_ptr[i], arc_ptr[i + 1]) for i in ids]).to(eng.device)
        out = walk_pool(wp[sel], wm[sel], mixed, 7)
        bound = _walk_bound(feat, traces, dmax, 7)
        for pos, i in enumerate(ids):
            one = wps.batch([i])
            sel1 = torch.arange(arc_ptr[i], arc_ptr[i + 1], device=eng.device)
            single = walk_pool(wp[sel1], wm[sel1], one, 7)[0]
            assert torch.equal(single[..., 1:], out[pos][..., 1:])
            assert bool(((single[..., 0] - out[pos][..., 0]).abs().cpu().double() <= bound[i][..., 0]).all())
            assert bool(((out[pos].cpu().double() - feat[i]).abs() <= bound[i]).all())


def test_walk_4096_nodes(eng):
    """The largest subgraph the kernels take (HBM flavour by default): a ring through all nodes, uniform weights,
    against scipy's sparse powers in fp64."""
    import scipy.sparse as ssp

    from s3grl_amd.walkpool import WalkPoolSplit, attention_weights, layout, walk_pool

    n = 4096
    edges = [(v, v + 1) for v in range(1, n - 1)] + [(0, n - 1), (0, 2)]
    wps = WalkPoolSplit(_make_list([(n, edges)], eng.device, x_width=1))
    b = wps.batch([0])
    assert layout(b.max_nodes, b.max_arcs, 1, 2)["forward"]["flavour"] == "hbm"
    z = torch.zeros((n, 1, 4), device=eng.device)
    wp, wm, _ = attention_weights(z, z, b)
    out = walk_pool(wp, wm, b, 2)
    out_lds = walk_pool(wp, wm, b, 2, lds_budget=159 << 10)
    assert torch.equal(out, out_lds)                          # W = 4 and 8 groups in both
    _, s, d, _, _ = _arcs(b)
    want = []
    for w in (wp, wm):
        P = ssp.csr_matrix((w.cpu().double().numpy()[:, 0], (d.numpy(), s.numpy())), shape=(n, n))
        X, rows = P, []
        for _ in range(2):
            X = X @ P
            rows.append((X.diagonal().sum(), X[0, 0] + X[1, 1], X[0, 1] + X[1, 0]))
        want.append(rows)
    got = out.cpu().double()[0, 0]
    for t in range(2):
        trp, trm = want[0][t][0], want[1][t][0]
        tol = (t + 2) * (3 + 2) * U
        assert abs(got[t, 0] - (trp - trm)) <= tol * (trp + trm)
        for col, (sign, idx) in zip((1, 2, 3, 4), ((0, 1), (1, 1), (0, 2), (1, 2))):
            assert abs(got[t, col] - want[sign][t][idx]) <= tol * abs(want[sign][t][idx])


# ---- backwards -----------------------------------------------------------------------------------------------------
def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max().clamp(min=1e-300)).item()


def _check_yardstick(what, gpu, cpu32, ref64):
    e_gpu, e_cpu = _rel(gpu, ref64), _rel(cpu32, ref64)
    print(f"{what}: GPU error {e_gpu:.3e}, fp32 restatement error {e_cpu:.3e}")
    assert e_gpu <= max(8 * e_cpu, FLOOR), what
    return e_gpu, e_cpu


BACKWARD_LISTS = ("hand", "rand300_h1", "usair_h1")


@pytest.mark.parametrize("hidden", [8, 32])
@pytest.mark.parametrize("heads", [1, 2, 3])
def test_attention_backward(eng, lists, heads, hidden):
    from s3grl_amd.walkpool import attention_weights

    for name in BACKWARD_LISTS:
        wps, graphs = lists[name]
        b = wps.batch(np.arange(len(wps)))
        gen = torch.Generator().manual_seed(9)
        q0 = torch.randn((b.num_nodes, heads, hidden), generator=gen)
        k0 = torch.randn((b.num_nodes, heads, hidden), generator=gen)
        gp, gm = torch.randn((b.num_arcs, heads), generator=gen), torch.randn((b.num_arcs, heads), generator=gen)
        go = torch.randn((len(wps), heads), generator=gen)
        link, s, d, _, _ = _arcs(b)
        grads = []
        for run in range(2):
            q, k = q0.to(eng.device).requires_grad_(), k0.to(eng.device).requires_grad_()
            wp, wm, om = attention_weights(q, k, b)
            ((wp * gp.to(eng.device)).sum() + (wm * gm.to(eng.device)).sum() + (om * go.to(eng.device)).sum()).backward()
            grads.append((q.grad.cpu(), k.grad.cpu()))
        assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
        ref = {}
        for dtype in (torch.float64, torch.float32):
            q, k = q0.to(dtype).requires_grad_(), k0.to(dtype).requires_grad_()
            loss, a = 0, 0
            for g, (n, src, dst) in enumerate(graphs):
                Pp, Pm, om, _ = R.attention_dense(q[a:a + n], k[a:a + n], n, src, dst)
                sel = link == g
                hh = torch.arange(heads)[None, :]
                loss = loss + (Pp[hh, d[sel][:, None], s[sel][:, None]] * gp[sel].to(dtype)).sum() \
                    + (Pm[hh, d[sel][:, None], s[sel][:, None]] * gm[sel].to(dtype)).sum() + (om * go[g].to(dtype)).sum()
                a += n
            loss.backward()
            ref[dtype] = (q.grad, k.grad)
        for i, what in enumerate(("dq", "dk")):
            _check_yardstick(f"attention {what} {name} heads {heads} hidden {hidden}", grads[0][i],
                             ref[torch.float32][i].double(), ref[torch.float64][i])


@pytest.mark.parametrize("heads", [1, 2, 3])
def test_walk_backward(eng, lists, walk_cases, heads):
    from s3grl_amd.walkpool import walk_pool

    for name in BACKWARD_LISTS:
        wps, graphs = lists[name]
        b, wp0, wm0, _, _, _ = walk_cases(name, heads)
        arcs = _arcs(b)
        link, s, d = arcs[:3]
        for walk_len in (1, 2, 7):
            gen = torch.Generator().manual_seed(13)
            gout = torch.randn((len(wps), heads, walk_len, 5), generator=gen)
            ref = {}
            for dtype in (torch.float64, torch.float32):
                wp, wm = wp0.cpu().to(dtype).requires_grad_(), wm0.cpu().to(dtype).requires_grad_()
                loss = 0
                for g, (n, _, _) in enumerate(graphs):
                    sel = link == g
                    Pp, Pm = (R.weights_to_dense(w[sel], n, s[sel], d[sel]) for w in (wp, wm))
                    loss = loss + (R.walk_features(Pp, Pm, walk_len)[0] * gout[g].to(dtype)).sum()
                loss.backward()
                ref[dtype] = (wp.grad, wm.grad)
            got = {}
            for lds in (0, _small_budget(b), 1):
                runs = []
                for run in range(2):
                    wp, wm = wp0.clone().requires_grad_(), wm0.clone().requires_grad_()
                    (walk_pool(wp, wm, b, walk_len, lds_budget=lds) * gout.to(eng.device)).sum().backward()
                    runs.append((wp.grad.cpu(), wm.grad.cpu()))
                assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
                got[lds] = runs[0]
                for i, what in enumerate(("d weights_p", "d weights_m")):
                    _check_yardstick(f"walk {what} {name} heads {heads} walk_len {walk_len} lds_budget {lds}",
                                     runs[0][i], ref[torch.float32][i].double(), ref[torch.float64][i])
            small = got[_small_budget(b)]
            assert torch.equal(small[0], got[1][0]) and torch.equal(small[1], got[1][1])      # W = 4, the same groups


# ---- the model -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def usair8(eng):
    """Eight USAir links (four train positives, four non-edges) at one hop, DRNL labels, 8 random features."""
    from s3grl_amd.seal import enclosing_subgraphs
    from s3grl_amd.walkpool import WalkPoolSplit

    n, e, A = _topology("usair")
    rng = np.random.default_rng(21)
    pos = e[rng.choice(len(e), 4, replace=False)]
    neg = np.array([[5, 77], [120, 9], [200, 31], [310, 2]])
    x = torch.from_numpy(rng.standard_normal((n, 8)).astype(np.float32))
    subs = enclosing_subgraphs(np.concatenate([pos, neg]).T, A, x, 0, 1, "drnl", engine=eng)
    y = torch.tensor([1.0] * 4 + [0.0] * 4)
    return WalkPoolSplit(subs), _graphs_of(subs), y


@pytest.mark.parametrize("drnl,MSE", [(True, False), (False, True)])
def test_model_teacher_forced(eng, usair8, drnl, MSE):
    from torch.nn import functional as F

    from s3grl_amd.walkpool import LinkPredTwin

    wps, graphs, y = usair8
    heads, walk_len, hid, F_in = 2, 7, 16, 8
    torch.manual_seed(4)
    twin = LinkPredTwin(F_in + (hid if drnl else 0), hid, heads, walk_len, drnl=drnl, z_max=100, MSE=MSE)
    state = {k: v.clone() for k, v in twin.state_dict().items()}
    twin.dropout = twin.wp.dropout = twin.classifier.dropout = 0.0          # the reference hard-codes 0.5
    twin.to(eng.device).train()
    batch = wps.batch(np.arange(8))
    xs = [batch.x[batch.node_ptr[g]:batch.node_ptr[g + 1]].cpu() for g in range(8)]
    zs = [batch.z[batch.node_ptr[g]:batch.node_ptr[g + 1]].cpu() for g in range(8)]
    assert max(int(z.max()) for z in zs) < 100

    def loss_of(out, target):
        return F.mse_loss(out.view(-1), target) if MSE else F.binary_cross_entropy_with_logits(out.view(-1), target)

    def train(model, forward, target):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = loss_of(forward(), target)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        return losses, {k: v.detach().cpu().double() for k, v in model.named_parameters()}

    out = twin(batch)
    assert out.shape == (8, 1)
    gpu_losses, gpu_params = train(twin, lambda: twin(batch), y.to(eng.device))
    res = {}
    for dtype in (torch.float64, torch.float32):
        ref = R.DenseLinkPred(F_in + (hid if drnl else 0), hid, heads, walk_len, drnl=drnl, z_max=100, MSE=MSE)
        ref.load_state_dict(state)
        ref.to(dtype).train()
        res[dtype] = train(ref, lambda: ref(graphs, [x.to(dtype) for x in xs], zs), y.to(dtype))
    l64, p64 = res[torch.float64]
    l32, p32 = res[torch.float32]
    print(f"losses fp64 {l64} GPU {gpu_losses} fp32 restatement {l32}")
    _check_yardstick(f"losses drnl {drnl} MSE {MSE}", torch.tensor(gpu_losses), torch.tensor(l32, dtype=torch.float64),
                     torch.tensor(l64, dtype=torch.float64))
    assert set(gpu_params) == set(p64)
    gpu_all = torch.cat([gpu_params[k].reshape(-1) for k in sorted(p64)])
    all32 = torch.cat([p32[k].reshape(-1) for k in sorted(p64)])
    all64 = torch.cat([p64[k].reshape(-1) for k in sorted(p64)])
    _check_yardstick(f"parameters drnl {drnl} MSE {MSE}", gpu_all, all32, all64)


def _usair200():
    """A 200-link subset of a USAir split: 70 + 70 training, 15 + 15 validation and 15 + 15 test links."""
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    full = W.edge_split(n, e, seed=0)
    take = {"train": 70, "valid": 15, "test": 15}
    links = {s: (full.links[s][0][:, ::7][:, :c], full.links[s][1][:, ::7][:, :c]) for s, c in take.items()}
    assert sum(p.shape[1] + q.shape[1] for p, q in links.values()) == 200
    return W.Split(n, full.train_edges, full.A, links)


def test_run_walkpool_drnl(eng):
    """With DRNL the label embedding stands beside x: conv1 and the attention encoder are hidden wider."""
    from s3grl_amd.walkpool import run_walkpool

    res = run_walkpool(_usair200(), epochs=2, lr=1e-3, drnl=True, hidden=16, embedding_dim=8, seed=1, device=eng.device)
    model = res["model"]
    assert model.conv1.lin.weight.shape == (16, 8 + 16) and model.wp.lin_key1.weight.shape == (16, 8 + 3 * 16)
    assert len(res["history"]) == 2
    assert all(math.isfinite(h["train_loss"]) and 0.0 <= h["val_auc"] <= 1.0 for h in res["history"])
    res_mse = run_walkpool(_usair200(), epochs=1, lr=1e-3, MSE=True, hidden=16, embedding_dim=8, seed=1,
                           device=eng.device)
    assert bool(((res_mse["scores"]["test"] >= 0) & (res_mse["scores"]["test"] <= 1)).all())   # the sigmoid's range


def test_run_walkpool_smoke(eng):
    from s3grl_amd.metrics import LinkMetrics
    from s3grl_amd.walkpool import run_walkpool

    split = _usair200()
    res = run_walkpool(split, epochs=3, lr=1e-3, seed=1, device=eng.device)
    hist = res["history"]
    assert len(hist) == 3
    assert set(hist[0]) == {"epoch", "train_loss", "val_loss", "val_auc", "val_ap", "test_auc", "test_ap"}
    print([(h["train_loss"], h["val_auc"], h["test_auc"]) for h in hist])
    assert hist[-1]["train_loss"] < hist[0]["train_loss"]
    m = LinkMetrics(eng.device)
    for name, key in (("valid", "val"), ("test", "test")):
        r = m.ranked(res["scores"][name], res["labels"][name])
        assert r["AUC"] == hist[-1][f"{key}_auc"] and r["AP"] == hist[-1][f"{key}_ap"]
    for pick in ("best_val_auc", "best_val_loss"):
        h = hist[res[pick]["epoch"] - 1]
        assert res[pick] == {"epoch": h["epoch"], "test_auc": h["test_auc"], "test_ap": h["test_ap"]}
    assert res["best_val_auc"]["epoch"] == min(h["epoch"] for h in hist if h["val_auc"] == max(x["val_auc"] for x in hist))


# ---- every column block, the backward beyond its register sums, general attention inputs ------------------------------
def _walk_against_restatement(eng, wps, graphs, ids, heads, walk_len, fwd_budgets, bwd_budgets, what):
    """walk_pool forward (the issue's bound) and backward (the fp32 yardstick) of the links `ids` as one batch, two
    runs bit-identical; returns {budget: features} and {budget: (d weights_p, d weights_m)}."""
    from s3grl_amd.walkpool import walk_pool

    b = wps.batch(ids)
    sub = [graphs[i] for i in ids]
    wp0, wm0 = _gpu_weights(eng, b, heads)
    arcs = _arcs(b)
    link, s, d = arcs[:3]
    both = [R.walk_features(p, m, walk_len) for p, m in zip(_dense_weights(sub, arcs, wp0.cpu(), torch.float64),
                                                           _dense_weights(sub, arcs, wm0.cpu(), torch.float64))]
    feat, traces = torch.stack([f for f, _ in both]), torch.stack([t for _, t in both])
    dmax = torch.tensor([int(arcs[4][link == g].max()) for g in range(len(ids))], dtype=torch.float64)
    bound = _walk_bound(feat, traces, dmax, walk_len)
    outs = {}
    for lds in fwd_budgets:
        out = walk_pool(wp0, wm0, b, walk_len, lds_budget=lds)
        assert torch.equal(out, walk_pool(wp0, wm0, b, walk_len, lds_budget=lds))
        err = (out.cpu().double() - feat).abs()
        print(f"{what} forward lds_budget {lds}: error / bound {(err / bound.clamp(min=1e-300))[bound > 0].max():.3f}")
        assert bool((err <= bound).all())
        outs[lds] = out
    gen = torch.Generator().manual_seed(17)
    gout = torch.randn((len(ids), heads, walk_len, 5), generator=gen)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        wp, wm = wp0.cpu().to(dtype).requires_grad_(), wm0.cpu().to(dtype).requires_grad_()
        loss = 0
        for g, (n, _, _) in enumerate(sub):
            sel = link == g
            Pp, Pm = (R.weights_to_dense(w[sel], n, s[sel], d[sel]) for w in (wp, wm))
            loss = loss + (R.walk_features(Pp, Pm, walk_len)[0] * gout[g].to(dtype)).sum()
        loss.backward()
        ref[dtype] = (wp.grad, wm.grad)
    grads = {}
    for lds in bwd_budgets:
        runs = []
        for _ in range(2):
            wp, wm = wp0.clone().requires_grad_(), wm0.clone().requires_grad_()
            (walk_pool(wp, wm, b, walk_len, lds_budget=lds) * gout.to(eng.device)).sum().backward()
            runs.append((wp.grad.cpu(), wm.grad.cpu()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        for i, name in enumerate(("d weights_p", "d weights_m")):
            _check_yardstick(f"{what} {name} lds_budget {lds}", runs[0][i], ref[torch.float32][i].double(),
                             ref[torch.float64][i])
        grads[lds] = runs[0]
    return b, outs, grads


@pytest.mark.parametrize("W", [4, 8, 16, 32])
def test_block_boundaries(eng, lists, W):
    """Subgraphs of W - 1, W and W + 1 nodes as one batch, at the budgets under which layout() reports the column block
    W for the forward and for the backward: every instantiation of both kernels, one node short of a block, a full
    block, and one node into the next."""
    from s3grl_amd.walkpool import layout

    wps, graphs = lists["hand"]
    heads, walk_len = 2, 2
    ids = [4 + HAND_SIZES.index(n) for n in (W - 1, W, W + 1)]
    assert [graphs[i][0] for i in ids] == [W - 1, W, W + 1]
    b = wps.batch(ids)
    fwd = 2 * (W + 1) * W * 4                                 # the forward's 2 arrays at W, nothing wider
    bwd = (walk_len + 2) * (W + 1) * W * 4                    # the backward's walk_len + 2 arrays at W
    assert layout(b.max_nodes, b.max_arcs, heads, walk_len, fwd)["forward"] == {
        "block": W, "groups": 2, "flavour": "lds", "workspace_bytes": 4 * heads * 2 * 2 * walk_len}
    lay = layout(b.max_nodes, b.max_arcs, heads, walk_len, bwd)["backward"]
    assert lay["block"] == W and lay["groups"] == 2 and lay["flavour"] == "lds"
    _, outs, grads = _walk_against_restatement(eng, wps, graphs, ids, heads, walk_len, (fwd, 1), (bwd, 1), f"block {W}")
    assert torch.equal(outs[fwd][..., 1:], outs[1][..., 1:])
    if W == 4:                                                # the HBM flavour has W = 4 too: the same order throughout
        assert torch.equal(outs[fwd], outs[1])
        assert torch.equal(grads[bwd][0], grads[1][0]) and torch.equal(grads[bwd][1], grads[1][1])


def test_walk_backward_beyond_register_sums(eng):
    """A backward thread keeps the sums of up to 20 of a link's arcs in registers (5 120 arcs per link); a link with more
    adds into its HBM slice instead.  A complete graph on 80 nodes without the link: 6 320 arcs of E+."""
    from s3grl_amd.walkpool import WalkPoolSplit

    n = 80
    edges = [(u, v) for u in range(n) for v in range(u + 1, n) if (u, v) != (0, 1)]
    subs = _make_list([(n, edges), (3, [(0, 2), (1, 2)])], eng.device)
    wps, graphs = WalkPoolSplit(subs), _graphs_of(subs)
    b, _, grads = _walk_against_restatement(eng, wps, graphs, [0, 1], 2, 7, (0, 1), (0, 1), "6320 arcs")
    assert b.max_arcs == 6320 and b.max_arcs > 20 * 256
    one = _walk_against_restatement(eng, wps, graphs, [0], 1, 2, (0,), (0, 1), "6320 arcs alone")[2]
    assert one[0][0].shape == (6320, 1)


@pytest.mark.parametrize("hidden", [8, 32])
def test_attention_forward_general_inputs(eng, lists, hidden):
    """q and k from a normal distribution: the dot product now rounds too.  Its fp32 error is at most
    hidden·2^-23·sum|q_i k_i|, so a logit is off by D = that / sqrt(hidden); a weight is exp(w_e) over a sum of such
    terms, so its relative error grows by at most |delta_e| + max|delta| <= 2·max D over the node's in-arcs, on top of
    the issue's (8 + deg_in + 4)·2^-23.  omega: sigmoid' <= 1/4, so (D_ij + D_ji) / 4 more."""
    from s3grl_amd.walkpool import attention_weights

    heads = 2
    for name in ("hand", "usair_h1"):
        wps, graphs = lists[name]
        b = wps.batch(np.arange(len(wps)))
        gen = torch.Generator().manual_seed(23)
        q = (0.5 * torch.randn((b.num_nodes, heads, hidden), generator=gen)).to(eng.device)
        k = torch.randn((b.num_nodes, heads, hidden), generator=gen).to(eng.device)
        wp, wm, om = attention_weights(q, k, b)
        ref = _attention_reference(graphs, q.cpu(), k.cpu(), torch.float64)
        link, s, d, mask, deg = _arcs(b)
        ei, _ = b.in_edge_index()
        ei = ei.cpu()
        q64, k64 = q.cpu().double(), k.cpu().double()
        logit = (q64[ei[0]] * k64[ei[1]]).sum(-1) / math.sqrt(hidden)
        assert float(logit.abs().max()) <= 8
        D = hidden * U * (q64[ei[0]].abs() * k64[ei[1]].abs()).sum(-1) / math.sqrt(hidden)       # [e, heads]
        Dmax = torch.zeros((b.num_nodes, heads), dtype=torch.float64).index_reduce(0, ei[1], D, "amax")[ei[1]]
        bound = ((8 + deg + 4) * U).double()[:, None] + 2 * Dmax
        ref_p = torch.stack([ref[g][0][:, c, r] for g, r, c in zip(link.tolist(), s.tolist(), d.tolist())])
        ref_m = torch.stack([ref[g][1][:, c, r] for g, r, c in zip(link.tolist(), s.tolist(), d.tolist())])
        err_p = ((wp.cpu().double() - ref_p).abs() / ref_p / bound).max().item()
        live = ref_m > 0
        err_m = ((wm.cpu().double() - ref_m).abs() / ref_m.clamp(min=1e-300) / bound)[live].max().item()
        Dcand = torch.zeros((len(wps), heads), dtype=torch.float64).index_add(0, link[~mask], D[~mask])
        err_o = ((om.cpu().double() - torch.stack([r[2] for r in ref])).abs() / ((8 + 4) * U + Dcand / 4)).max().item()
        print(f"attention on normal inputs {name} hidden {hidden}: error / bound p {err_p:.3f} m {err_m:.3f} "
              f"omega {err_o:.3f}")
        assert bool((wm.cpu()[~mask] == 0).all())
        assert max(err_p, err_m, err_o) <= 1.0
