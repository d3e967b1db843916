"""-m gpu: the LDS of the link classes and the coefficients no kernel loads.

1. A link gives the same integers and the same row bits whatever class (LDS need, thread count, HBM scratch)
   it is planned into — across the class bounds cut by what fits a CU, with one link exactly at a cut bound
   and one the smallest step (one list entry, 4 bytes) above it.
2. The deferred-hub bitmap is part of a link's LDS only on graphs that arm the hub path: the same topology
   armed (one node of 300 neighbours) and disarmed gives the same rows for the links out of that node's reach.
3. The link kernels no longer store a middle operator's zeros beyond the prefix the gather multiplies them
   over.  A plan whose coefficient block was used before (every entry non-zero) must give the rows, bit for
   bit, of a fresh engine: nobody reads what is no longer written.

Small graphs only.  The bounds are restated here from s3grl_link_classes.hpp (cut_bounds) and checked against
the class counts the engine reports under S3GRL_DEBUG."""
import re

import numpy as np
import pytest
import scipy.sparse as ssp

import oracle
from conftest import csr_from_undirected

pytestmark = pytest.mark.gpu

TOL = 1e-5            # the project's parity bar (tests/test_gpu_parity.py)
ATOL = 1e-10


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=-1, keepdims=True))
    return float(np.max(np.clip(np.abs(got - ref) - ATOL, 0, None) / np.maximum(scale, 1e-30)))


def new_engine():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    return Engine("cuda:0")


@pytest.fixture(scope="module")
def eng():
    e = new_engine()
    yield e
    e.close()


def random_edges(n, m, seed):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(m, 2))
    e = e[e[:, 0] != e[:, 1]]
    return np.unique(np.sort(e, axis=1), axis=0)


def balls(A, src, dst, hops):
    """|ball_d({src, dst})| for d = 0..hops on the unmasked graph (the engine's hop-major list prefixes)."""
    seen = {int(src), int(dst)}
    fringe = set(seen)
    out = [len(seen)]
    for _ in range(hops):
        nxt = set()
        for v in fringe:
            nxt.update(A.indices[A.indptr[v]:A.indptr[v + 1]].tolist())
        fringe = nxt - seen
        seen |= fringe
        out.append(len(seen))
    return out


# ---- the class bounds, restated (s3grl_link_classes.hpp) ---------------------------------------------
LDS, GRAN, MAX_LEVELS, HUB_WORDS, HUB_ARM = 163840, 1280, 32, 256, 256
NOMINAL = [6144, 12288, 24576, 49152, 98304, 163840]


def fixed_bytes(num_nodes, cn_cap, K, hubs):
    return 4 * (3 * ((num_nodes + 31) // 32) + cn_cap + MAX_LEVELS + 4 * K + 32 + (HUB_WORDS if hubs else 0))


def share(k):
    return LDS // k // GRAN * GRAN


def cut_bounds(fixed, avail):
    b = []
    for nom in NOMINAL:
        k0 = max(1, LDS // (fixed + nom))
        lo, hi = share(k0 + 1) - fixed, share(k0) - fixed
        v = nom
        if hi > 0:
            v = lo if (lo > 0 and nom - lo < hi - nom) else hi
        b.append(min(v, avail))
    b[-1] = avail
    return b


def need_of(n, p):
    return 4 * n + 20 * p + 16


def class_of(need, bounds):
    return sum(need > b for b in bounds)   # len(bounds) = the HBM-scratch class


def debug_classes(capfd):
    """class counts of the plans created since the last call ([s3grl] ... classes: c0 c1 ...)"""
    err = capfd.readouterr().err
    return [[int(t) for t in m.group(1).split()] for m in re.finditer(r"classes:((?: \d+)+)", err)]


def plan_outputs(eng, G, L, f, **kw):
    plan = eng.plan(G, L, **kw)
    rows = plan.run(f)
    out = (rows, plan.row_ptr(), plan.row_nodes(), plan.export_subgraphs(), dict(plan.stats))
    plan.close()
    return out


def assert_same_outputs(a, b):
    import torch

    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])               # row_ptr, row nodes
    for x, y in zip(a[3], b[3]):                                             # node lists and hop distances
        assert torch.equal(x, y)
    # bit for bit: compared as integers, so that a NaN cannot hide
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    for k in a[4]:
        if k != "workspace_bytes":
            assert a[4][k] == b[4][k], k


# ---- 1. class invisibility across the cut bounds ------------------------------------------------------
@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
def test_classes_invisible_small_graph(eng, monkeypatch, mode):
    """~300 nodes: the direct-map classes, the bitmap classes (S3GRL_NO_DM) and, with the LDS budget shrunk,
    other bitmap classes, other thread counts and the HBM-scratch class: same integers, same row bits."""
    n = 300
    A = csr_from_undirected(n, random_edges(n, 700, 5))
    X = np.random.default_rng(6).standard_normal((n, 21))
    links = np.random.default_rng(7).integers(0, n, size=(64, 2))
    links = links[links[:, 0] != links[:, 1]]
    G = eng.graph(A)
    f = eng.features(X)
    L = eng.links(links.T.copy())
    kw = dict(mode=mode, num_hops=2, sign_k=2)
    ref = plan_outputs(eng, G, L, f, **kw)
    monkeypatch.setenv("S3GRL_NO_DM", "1")
    assert_same_outputs(ref, plan_outputs(eng, G, L, f, **kw))
    for budget in ("3000", "1200", "400"):
        monkeypatch.setenv("S3GRL_LDS_BUDGET", budget)
        assert_same_outputs(ref, plan_outputs(eng, G, L, f, **kw))
    G.close()


def _gadget(edges, free, a, b, hop1, leaves):
    """link (a, b): `hop1` neighbours of a, `leaves` nodes at hop 2 spread over them (at most 200 each: no row
    arms the hub path).  n = 2 + hop1 + leaves, and with sign_k = 2 the prefix p = 2 + hop1."""
    mids = [free.pop() for _ in range(hop1)]
    edges += [[a, m] for m in mids]
    for i in range(leaves):
        edges.append([mids[i % hop1], free.pop()])
    assert leaves <= 200 * hop1


def test_classes_invisible_at_the_cut_bounds(eng, monkeypatch, capfd):
    """10 240 nodes (bitmap flavour, W = 320), num_hops 2, sign_k 2.  Two links sit at the first cut bound — one
    whose LDS need equals it, one a list entry above — and land in classes 0 and 1; every class count the engine
    reports equals the one worked out here from the restated bounds.  With the budget shrunk the same links run in
    other classes, with other thread counts and from HBM scratch: same integers, same row bits.
    (No link reaches the HBM-scratch class under the default bounds: without a hub row a subgraph of this graph
    needs at most ~50 KB.  The budget runs put most links there.)"""
    n, K, hops = 10240, 2, 2
    fixed = fixed_bytes(n, 1, K, False)
    bounds = cut_bounds(fixed, LDS - fixed)
    assert bounds[0] % 4 == 0 and 5000 < bounds[0] < 7000
    base = random_edges(7000, 9500, 11)           # nodes 7000.. are free for the gadgets
    edges = base.tolist()
    free = list(range(n - 1, 7003, -1))
    hop1 = 10
    leaves_at = (bounds[0] - 16 - 24 * (2 + hop1)) // 4       # need_of(2 + hop1 + leaves, 2 + hop1) == bounds[0]
    assert need_of(2 + hop1 + leaves_at, 2 + hop1) == bounds[0]
    _gadget(edges, free, 7000, 7001, hop1, leaves_at)          # exactly at the bound: class 0
    _gadget(edges, free, 7002, 7003, hop1, leaves_at + 1)      # one entry (4 bytes) above it: class 1
    A = csr_from_undirected(n, np.array(edges))
    assert np.diff(A.indptr).max() <= HUB_ARM                  # the hub path stays disarmed
    rng = np.random.default_rng(12)
    links = rng.integers(0, 7000, size=(62, 2))
    links[links[:, 0] == links[:, 1], 1] += 1
    links = np.concatenate([links, [[7000, 7001], [7002, 7003]]])
    want = [0] * 7
    for s, d in links:
        bl = balls(A, s, d, hops)
        want[class_of(need_of(bl[hops], bl[min(K - 1, hops)]), bounds)] += 1
    assert want[0] > 0 and want[1] > 0 and want[6] == 0
    assert need_of(*[balls(A, 7000, 7001, 2)[i] for i in (2, 1)]) == bounds[0]
    assert need_of(*[balls(A, 7002, 7003, 2)[i] for i in (2, 1)]) == bounds[0] + 4

    X = rng.standard_normal((n, 9))
    G = eng.graph(A)
    f = eng.features(X)
    L = eng.links(links.T.copy())
    kw = dict(mode="pos", num_hops=hops, sign_k=K, fold_reversed=False)
    monkeypatch.setenv("S3GRL_DEBUG", "1")
    capfd.readouterr()
    ref = plan_outputs(eng, G, L, f, **kw)
    got = debug_classes(capfd)
    assert got and got[-1][:7] == want, (got, want)
    for budget in ("20000", str(bounds[0] - 4), "2000"):
        monkeypatch.setenv("S3GRL_LDS_BUDGET", budget)
        assert_same_outputs(ref, plan_outputs(eng, G, L, f, **kw))
        got = debug_classes(capfd)[-1]
        cut = cut_bounds(fixed, min(LDS - fixed, int(budget)))
        want_b = [0] * 7
        for s, d in links:
            bl = balls(A, s, d, hops)
            want_b[class_of(need_of(bl[hops], bl[min(K - 1, hops)]), cut)] += 1
        assert got[:7] == want_b, (budget, got, want_b)
        if budget != "20000":
            assert want_b[6] > 0                  # the HBM-scratch class is in use
    G.close()


# ---- 2. hub path armed / disarmed ----------------------------------------------------------------------
def test_hub_words_only_where_the_hub_path_is_armed(eng):
    """The same 600-node topology twice: as it is (largest row far below 256 entries: no hub bitmap in a link's
    LDS), and with node 500 given 300 new neighbours (armed: the bitmap is there, list[] sits 1 KiB further on).
    Links whose 2-hop subgraph stays clear of that node's 3-hop ball have the same subgraph in both graphs and
    must give identical rows; every link of both graphs meets the oracle."""
    import torch

    n, hops, K = 1000, 2, 3
    base = random_edges(600, 1100, 21)
    hub = 500
    extra = np.array([[hub, v] for v in range(600, 900)])
    A0 = csr_from_undirected(n, base)
    A1 = csr_from_undirected(n, np.concatenate([base, extra]))
    assert np.diff(A0.indptr).max() < 32 and np.diff(A1.indptr).max() > HUB_ARM
    reach = ssp.csgraph.shortest_path(A1, unweighted=True, indices=[hub])[0]
    far = np.flatnonzero(reach[:600] > 3 + hops)          # their 2-hop balls miss the hub's 3-hop ball
    assert len(far) >= 40
    rng = np.random.default_rng(22)
    clear = rng.choice(far, size=(24, 2))
    clear = clear[clear[:, 0] != clear[:, 1]]
    near = np.array([[hub, 3], [hub, 600], [601, 602], [int(A1.indices[A1.indptr[hub]]), 7]])
    links = np.concatenate([clear, near])
    X = rng.standard_normal((n, 13)).astype(np.float32).astype(np.float64)
    outs = []
    for A in (A0, A1):
        G = eng.graph(A)
        f = eng.features(X)
        per_mode = {}
        for mode, fn in (("pos", oracle.get_PoS_prepped_ds), ("pos_plus", oracle.get_PoS_Plus_prepped_ds)):
            res = eng.precompute(G, f, eng.links(links.T.copy()), mode=mode, num_hops=hops, sign_k=K)
            ref, ref_ptr, _ = oracle.collate_rows(
                fn(links.T, hops, A, X, 1, {"sign_k": K, "k_node_set_strategy": "intersection"}, dtype=np.float64), K)
            np.testing.assert_array_equal(res.row_ptr.cpu().numpy(), ref_ptr)
            err = rel_err(res.rows.cpu().numpy(), ref)
            print(f"[hub words] max degree {np.diff(A.indptr).max()} {mode}: rel err {err:.2e}")
            assert err < TOL
            per_mode[mode] = res
        outs.append(per_mode)
        G.close()
    for mode in ("pos", "pos_plus"):
        r0, r1 = outs[0][mode], outs[1][mode]
        e0, e1 = int(r0.row_ptr[len(clear)]), int(r1.row_ptr[len(clear)])
        assert e0 == e1 and torch.equal(r0.row_ptr[:len(clear) + 1], r1.row_ptr[:len(clear) + 1])
        assert torch.equal(r0.row_nodes[:e0], r1.row_nodes[:e0])
        assert torch.equal(r0.rows[:e0].view(torch.int32), r1.rows[:e0].view(torch.int32))


# ---- 3. nobody reads what is no longer written ---------------------------------------------------------
def _poison(eng, nbytes, K, copies=32):
    """Runs and closes plans whose coefficient blocks have at least `nbytes` bytes, every entry written and (but
    for the masked target link) positive: one-hop plans on a clique, where every operator reaches every node.
    The arena keeps the blocks and hands each to the next request it fits best — `copies` of them, alive at the
    same time, so that the requests a plan makes before it asks for its coefficients do not use them up."""
    m = 40
    A = ssp.csr_matrix(np.ones((m, m)) - np.eye(m))
    pairs = np.array([[i, j] for i in range(m) for j in range(i + 1, m)])
    count = -(-nbytes // (m * K * 8))
    links = pairs[np.arange(count) % len(pairs)]
    G = eng.graph(A)
    L = eng.links(links.T.copy())
    plans = [eng.plan(G, L, mode="pos", num_hops=1, sign_k=K, fold_reversed=False) for _ in range(copies)]
    for plan in plans:
        assert plan.stats["total_support"] == count * m     # (reading the totals waits for the link kernels)
    for plan in plans:
        plan.close()
    G.close()


def _deep_graph():
    """400 nodes of mean degree 4: the balls of a link keep growing up to hop 3; node 399 isolated"""
    n = 400
    return n, csr_from_undirected(n, random_edges(399, 800, 31))


def _deep_links(n):
    rng = np.random.default_rng(32)
    links = rng.integers(0, n - 1, size=(48, 2))
    links[links[:, 0] == links[:, 1], 1] += 1
    return np.concatenate([links, links[:4, ::-1],        # reversed duplicates (folded into their twins)
                           [[n - 1, 5], [7, n - 1]]])     # an isolated endpoint


def _coef_bytes(A, links, hops, K, plus):
    """Upper bound of a plan's coefficient block, worked out on the CPU: K float2 per list entry of every row
    pair — PoS lays a link's one pair out over its whole node list, |ball(num_hops)|; PoS Plus adds one pair per
    two common neighbours.  (Sizing the plan on the engine itself would leave a block of exactly its size
    behind, full of its own values.)"""
    tot = 0
    for s, d in links:
        pairs = 1
        if plus:
            cn = np.intersect1d(A.indices[A.indptr[s]:A.indptr[s + 1]], A.indices[A.indptr[d]:A.indptr[d + 1]])
            pairs += (len(cn) + 1) // 2
        tot += pairs * balls(A, s, d, hops)[hops]
    return tot * K * 8


def _unwritten_entries(A, links, hops, K, row_hop):
    """Σ over links of the list entries of the LAST middle operator that lie beyond the zero fill: its limit is
    |ball(K - 1 + row_hop)|, the zeros go on for 3 entries (one gather group), the list for |ball(K + row_hop)|."""
    tot = 0
    for s, d in links:
        bl = balls(A, s, d, hops)
        lim = bl[min(K - 1 + row_hop, hops)]
        sup = bl[min(K + row_hop, hops)]
        tot += max(0, sup - (lim + 3))
    return tot


FEATURE_MODES = [("auto", 72, True), ("packed_only", 72, True), ("dense", 72, False),   # dense, F <= 128: narrow gather
                 ("dense", 300, False), ("sparse", 72, True)]


def _features_for(n, F, sparse_x, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, F)).astype(np.float32)
    if sparse_x:
        X *= rng.random((n, F)) < 0.06
    return X


@pytest.mark.parametrize("fmode,F,sparse_x", FEATURE_MODES)
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
def test_stale_coefficients_are_never_read(mode, K, fmode, F, sparse_x):
    """num_hops 3 with sign_k 2 and 3 (sign_k - 1 < num_hops: the middle operators stop short of the list), PoS
    and PoS Plus (common-neighbour pairs, row_hop 1), reversed duplicates, an isolated endpoint; packed rows with
    and without element rows, the narrow and the wide dense gather, sparse rows.  On one engine a one-hop clique
    plan first fills a coefficient block with non-zero values and closes; the deep plan then gets that block back.
    Its rows must equal, bit for bit, those of a fresh engine."""
    import torch

    hops = 3
    n, A = _deep_graph()
    links = _deep_links(n)
    # the case proves something only if operators stop short of their lists: checked here on the CPU
    assert _unwritten_entries(A, links, hops, K, 0) > 500
    X = _features_for(n, F, sparse_x, 33)
    results = []
    for poisoned in (True, False):
        e = new_engine()
        G = e.graph(A)
        f = e.features(X, mode=fmode)
        assert f.is_packed == (fmode in ("auto", "packed_only")) and f.is_sparse == (fmode == "sparse")
        L = e.links(links.T.copy())
        if poisoned:
            _poison(e, _coef_bytes(A, links, hops, K, mode == "pos_plus"), K)
        res = e.precompute(G, f, L, mode=mode, num_hops=hops, sign_k=K)
        results.append((res.rows.clone(), res.row_ptr.clone(), res.row_nodes.clone()))
        assert res.stats["folded_links"] == 4
        e.close()
    (r1, p1, n1), (r0, p0, n0) = results
    assert torch.equal(p1, p0) and torch.equal(n1, n0)
    assert torch.isfinite(r0).all()
    assert torch.equal(r1.view(torch.int32), r0.view(torch.int32))


@pytest.mark.parametrize("fmode,F,sparse_x", [("auto", 72, True), ("dense", 72, False), ("dense", 300, False)])
@pytest.mark.parametrize("K", [2, 3])
def test_stale_coefficients_of_a_split_list(K, fmode, F, sparse_x):
    """A star of 4 200 leaves, 60 of them with a pendant node: the list of a leaf-to-leaf link is longer than
    kSplitThreshold (4 096), so it is laid out and gathered in pieces and summed by combine_kernel.  sign_k 2:
    operator 1 stops at the centre (3 entries); sign_k 3: operator 2 stops at the leaves, the pendants are the
    last operator's alone."""
    import torch

    hops = 3
    leaves = 4200
    n = 1 + leaves + 60
    edges = [[0, v] for v in range(1, leaves + 1)] + [[100 + i, leaves + 1 + i] for i in range(60)]
    A = csr_from_undirected(n, np.array(edges))
    links = np.array([[1, 2], [3, 4000], [4000, 3], [0, 9], [150, 151]])
    for s, d in links[:2]:
        assert balls(A, s, d, hops)[min(K, hops)] > 4096
    assert _unwritten_entries(A, links, hops, K, 0) > 40
    X = _features_for(n, F, sparse_x, 41)
    results = []
    for poisoned in (True, False):
        e = new_engine()
        G = e.graph(A)
        f = e.features(X, mode=fmode)
        L = e.links(links.T.copy())
        if poisoned:
            _poison(e, _coef_bytes(A, links, hops, K, False), K)
        res = e.precompute(G, f, L, mode="pos", num_hops=hops, sign_k=K)
        results.append((res.rows.clone(), res.row_ptr.clone()))
        e.close()
    (r1, p1), (r0, p0) = results
    assert torch.equal(p1, p0) and torch.isfinite(r0).all()
    assert torch.equal(r1.view(torch.int32), r0.view(torch.int32))
