"""-m gpu: the neighbour visit of link_kernel's bitmap flavour.

The bitmap flavour keeps one record {inP, rank prefix, vis} per 32 nodes, reads a non-member's rank without a clamp
(the state arrays have a spare entry at index p), compares a neighbour against the masked partner only on list rows
0 and 1, and takes "the state counts" from the bit of P alone.  None of it may change a bit of the output.

One graph of 10 240 nodes (W = 320: bitmap flavour), num_hops 3, sign_k 2 and 3, PoS and PoS Plus:

* two tree gadgets whose hops 1, 2 and 3 each hold rows of 1, 4, 5, 8, 9, 16 and 17 stored neighbours (slot and pair
  edges of the walk with four lanes per row: 4 = the first slots, 8 = both slots, 16 = one step of the long-row
  loop, each plus one); their hop-3 rows reach on to hop 4, outside the subgraph.  One gadget's endpoints are
  adjacent (the mask is active), the other's are not.  A row of 0 stored neighbours is an isolated endpoint: a node
  the BFS reaches has a neighbour (the directed case below walks predecessor rows, which may be empty at any hop);
* endpoint pairs with 0 ... 17 stored neighbours each, adjacent (the partner is one of them) and not;
* a pair adjacent to nothing but each other: |P| = n = 2; with sign_k 3 the PoS Plus pairs reach the whole
  list (|P| = n), with sign_k 2 the lists end two hops beyond P;
* endpoints at bit 0 and bit 31 of bitmap word 0 and of word W - 1, both in the ids the engine walks by (rank of
  (degree descending, id ascending)) and, with the relabelling off, in the caller's ids;
* random links of the sparse base graph, one of them again reversed (folded into its twin).

Checked on the CPU first: the hops of the gadget links hold the row lengths claimed, the endpoints sit at the bits
claimed.  Then: integer outputs and the oracle at the parity tolerance; bit for bit against the hash flavour, the
direct-map flavour on the same topology squeezed into 2 048 ids, the HBM-scratch class (LDS budget; also with the
bitmaps' records in HBM), and with the relabelling off.  A directed graph of the same nodes against the oracle and its own HBM-scratch run.

The hash flavour sums a link whose every operator reaches the whole list (p == n, at most 512 nodes) through its
adjacency bit matrix, in another order (link_kernel, use_bm): those links are compared at the parity tolerance, the
others bit for bit."""
import numpy as np
import pytest

import oracle
from conftest import csr_from_arcs, csr_from_undirected
from test_gpu_link_lds_and_coefs import (TOL, assert_same_outputs, balls, debug_classes, plan_outputs, random_edges,
                                         rel_err)

gpu = pytest.mark.gpu

N, W, HOPS = 10240, 320, 3
LENGTHS = (1, 4, 5, 8, 9, 16, 17)
BASE = 1200          # the random base graph lives on ids below; gadgets and pairs on the free ids above
KW = lambda K: {"sign_k": K, "k_node_set_strategy": "intersection"}   # noqa: E731


def _tree(edges, free, a):
    """Below a: one node per length in LENGTHS at hop 1 (a itself + length - 1 children), among the children of hop 1
    one node per length at hop 2, among theirs one per length at hop 3 (whose children lie at hop 4)."""
    pool = []
    for d in LENGTHS:
        m = free.pop()
        edges.append([a, m])
        pool.append((m, d))
    for _ in range(3):
        children = []
        for m, d in pool:
            for _ in range(d - 1):
                c = free.pop()
                edges.append([m, c])
                children.append(c)
        assert len(children) >= len(LENGTHS)
        pool = list(zip(children[:len(LENGTHS)], LENGTHS))      # the others stay leaves


def _star(edges, free, d, partner=None):
    """a node with d stored neighbours: leaves, and `partner` as one of them"""
    s = free.pop()
    if partner is not None:
        edges.append([s, partner])
    for _ in range(d - (partner is not None)):
        edges.append([s, free.pop()])
    return s


def _build():
    edges = random_edges(BASE, 1700, 11).tolist()
    free = list(range(N - 40, BASE, -1))           # ids N-40 .. N-1 stay isolated: the tail of the degree order
    links = []
    a, b = free.pop(), free.pop()                  # gadget 1: adjacent endpoints
    edges.append([a, b])
    _tree(edges, free, a)
    _tree(edges, free, b)
    links.append([a, b])
    a2, b2 = free.pop(), free.pop()                # gadget 2: not adjacent; a path of two keeps them in one subgraph
    mid = free.pop()
    edges += [[a2, mid], [mid, b2]]
    _tree(edges, free, a2)
    links.append([b2, a2])
    gadget_links = list(links)
    lens = (0,) + LENGTHS
    for i in range(0, len(lens), 2):               # endpoints of every length, not adjacent
        links.append([_star(edges, free, lens[i]), _star(edges, free, lens[i + 1])])
    for d in LENGTHS[1:]:                          # ... and adjacent: the partner is one of the d
        y = _star(edges, free, d - 1)
        links.append([_star(edges, free, d, partner=y), y])
    u, v = free.pop(), free.pop()                  # adjacent to nothing but each other: n = p = 2
    edges.append([u, v])
    links.append([u, v])
    A = csr_from_undirected(N, np.array(edges))
    assert np.diff(A.indptr).max() <= 256          # the hub path stays disarmed
    deg = np.diff(A.indptr)
    order = np.lexsort((np.arange(N), -deg))       # order[new id] = caller's id (s3grl_relabel.hip)
    bit_nodes = [0, 31, N - 32, N - 1]
    links += [[order[0], order[N - 1]], [order[31], order[N - 32]], [0, N - 1], [31, N - 32]]
    rng = np.random.default_rng(12)
    rnd = rng.integers(0, BASE, size=(20, 2))
    rnd[rnd[:, 0] == rnd[:, 1], 1] += 1
    links = np.concatenate([np.array(links), rnd, rnd[:1, ::-1]])     # the last: a reversed duplicate
    return A, links, gadget_links, order, bit_nodes


def _hops_of(A, s, d):
    """nodes per hop of the BFS from {s, d} on the unmasked graph"""
    seen = {int(s), int(d)}
    levels = [sorted(seen)]
    for _ in range(HOPS):
        nxt = set()
        for v in levels[-1]:
            nxt.update(A.indices[A.indptr[v]:A.indptr[v + 1]].tolist())
        nxt -= seen
        if not nxt:
            break
        seen |= nxt
        levels.append(sorted(nxt))
    return levels


@pytest.fixture(scope="module")
def shape():
    A, links, gadget_links, order, bit_nodes = _build()
    return dict(A=A, links=links, gadget_links=gadget_links, order=order, bit_nodes=bit_nodes)


@pytest.fixture(scope="module")
def case(shape):
    A, links = shape["A"], shape["links"]
    X = np.random.default_rng(13).standard_normal((N, 11)).astype(np.float32).astype(np.float64)
    ref = {}
    for mode, fn in (("pos", oracle.get_PoS_prepped_ds), ("pos_plus", oracle.get_PoS_Plus_prepped_ds)):
        for K in (2, 3):
            ref[mode, K] = oracle.collate_rows(fn(links.T, HOPS, A, X, 1, KW(K), dtype=np.float64), K)[:2]
    return dict(shape, X=X, ref=ref)


@pytest.fixture(scope="module")
def eng():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    e = Engine("cuda:0")
    yield e
    e.close()


def test_shapes_hold_what_they_claim(shape):
    """No GPU: row lengths per hop, bit positions, the sizes of P of the graph the cases below run on."""
    case = shape
    A, links = case["A"], case["links"]
    deg = np.diff(A.indptr)
    for s, d in case["gadget_links"]:
        levels = _hops_of(A, s, d)
        assert len(levels) == HOPS + 1
        for h in (1, 2, 3):
            assert set(LENGTHS) <= set(deg[levels[h]].tolist()), (s, d, h)
        # hop 3 reaches on: stored neighbours outside the subgraph
        inside = set(sum(levels, []))
        assert any(int(u) not in inside for v in levels[3] for u in A.indices[A.indptr[v]:A.indptr[v + 1]])
    ends = deg[links.ravel()]
    assert set((0,) + LENGTHS) <= set(ends.tolist())
    adjacent = [bool(A[s, d]) for s, d in links]
    assert any(adjacent) and not all(adjacent)
    for want in (4, 5, 8, 9, 16, 17):              # the masked partner inside rows of every length
        assert any(adj and deg[s] == want for (s, d), adj in zip(links, adjacent))
    # bits 0 and 31 of words 0 and W - 1 hold endpoints: in the walk order and in the caller's ids
    new_of_old = np.empty(N, dtype=np.int64)
    new_of_old[case["order"]] = np.arange(N)
    assert set(case["bit_nodes"]) <= set(new_of_old[links.ravel()].tolist())
    assert set(case["bit_nodes"]) <= set(links.ravel().tolist())
    assert [b >> 5 for b in case["bit_nodes"]] == [0, 0, W - 1, W - 1] and [b & 31 for b in case["bit_nodes"]] == [0, 31, 0, 31]
    sizes = [balls(A, s, d, HOPS) for s, d in links]
    assert any(bl[HOPS] == 2 for bl in sizes)                           # |P| = n = 2
    assert any(bl[HOPS] > 2 and bl[2] == bl[HOPS] for bl in sizes)      # sign_k 3: |P| = n > 2
    assert any(bl[2] < bl[HOPS] for bl in sizes)                        # P a proper prefix at both sign_k
    assert (links[-1] == links[-21][::-1]).all()                       # the reversed duplicate of the first random link


def _full_reach(A, links, K, plus):
    """per link: does every operator reach the whole list (p == n)?"""
    out = []
    for s, d in links:
        bl = balls(A, s, d, HOPS)
        row_hop = 0
        if plus:
            cn = np.intersect1d(A.indices[A.indptr[s]:A.indptr[s + 1]], A.indices[A.indptr[d]:A.indptr[d + 1]])
            row_hop = 1 if len(np.setdiff1d(cn, [s, d])) or A[s, s] or A[d, d] else 0
        out.append(bl[min(K - 1 + row_hop, HOPS)] == bl[HOPS])
    return np.array(out)


def _same_but_full_reach(a, b, full):
    """assert_same_outputs, with the rows of the links flagged in `full` at the parity tolerance"""
    import torch

    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for x, y in zip(a[3], b[3]):
        assert torch.equal(x, y)
    ptr = a[1].cpu().numpy()
    ra, rb = a[0].cpu().numpy(), b[0].cpu().numpy()
    for l, f in enumerate(full):
        x, y = ra[ptr[l]:ptr[l + 1]], rb[ptr[l]:ptr[l + 1]]
        if f:
            assert rel_err(x, y) < TOL, l
        else:
            assert np.array_equal(x.view(np.int32), y.view(np.int32)), l


@gpu
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
def test_visit_against_oracle_and_untouched_flavours(eng, case, monkeypatch, capfd, mode, K):
    import torch

    A, links, X = case["A"], case["links"], case["X"]
    kw = dict(mode=mode, num_hops=HOPS, sign_k=K)
    ref_rows, ref_ptr = case["ref"][mode, K]
    full = _full_reach(A, links, K, mode == "pos_plus")

    def run(graph, feats, lk):
        return plan_outputs(eng, graph, lk, feats, **kw)

    G, f, L = eng.graph(A), eng.features(X), eng.links(links.T.copy())
    monkeypatch.setenv("S3GRL_DEBUG", "1")
    capfd.readouterr()
    got = run(G, f, L)
    classes = debug_classes(capfd)[-1]
    assert sum(classes[:6]) >= len(links) - 1 and classes[6] == 0     # LDS classes of the bitmap flavour (one link folded)
    np.testing.assert_array_equal(got[1].cpu().numpy(), ref_ptr)
    err = rel_err(got[0].cpu().numpy(), ref_rows)
    print(f"[link visit] {mode} K={K}: rel err {err:.2e}")
    assert err < TOL
    assert got[4]["folded_links"] == 1
    # the HBM-scratch class: list and state in a slice of HBM, same bits
    monkeypatch.setenv("S3GRL_LDS_BUDGET", "400")
    scratch = run(G, f, L)
    assert debug_classes(capfd)[-1][6] > 0
    assert_same_outputs(got, scratch)
    monkeypatch.setenv("S3GRL_FORCE_EXT_BITMAPS", "1")                # ... and the records of the bitmaps too
    assert_same_outputs(got, run(G, f, L))
    monkeypatch.delenv("S3GRL_FORCE_EXT_BITMAPS")
    monkeypatch.delenv("S3GRL_LDS_BUDGET")
    # the relabelling off: the caller's ids are the bitmap's; other sums (another row order), the same integers
    monkeypatch.setenv("S3GRL_NO_RELABEL", "1")
    plain = run(G, f, L)
    assert torch.equal(plain[1], got[1]) and torch.equal(plain[2], got[2])
    for x, y in zip(plain[3], got[3]):
        assert torch.equal(x, y)
    assert rel_err(plain[0].cpu().numpy(), ref_rows) < TOL
    monkeypatch.setenv("S3GRL_FORCE_HASH", "1")
    Gh = eng.graph(A)
    _same_but_full_reach(plain, run(Gh, f, L), full)
    monkeypatch.delenv("S3GRL_NO_RELABEL")
    # the hash flavour on the relabelled graph
    _same_but_full_reach(got, run(Gh, f, L), full)
    monkeypatch.delenv("S3GRL_FORCE_HASH")
    Gh.close()
    G.close()
    # the direct map: the same topology on 2 048 ids, order kept (so the walk order, the rows and the lists keep theirs;
    # a map of 4 KB pays in every class, dm_class_mask_for: at 8 192 ids only links of 24 KB and more would take it)
    NS = 2048
    used = np.flatnonzero(np.diff(A.indptr) > 0)
    used = np.union1d(used, links.ravel())
    assert len(used) <= NS
    small_of = np.full(N, -1, dtype=np.int64)
    small_of[used] = np.arange(len(used))
    coo = A.tocoo()
    As = csr_from_arcs(NS, np.stack([small_of[coo.row], small_of[coo.col]], axis=1))
    Xs = np.zeros((NS, X.shape[1]))
    Xs[:len(used)] = X[used]
    Gs = eng.graph(As)
    dm = run(Gs, eng.features(Xs), eng.links(small_of[links].T.copy()))
    dm_classes = debug_classes(capfd)[-1]
    assert torch.equal(dm[1], got[1])
    back = torch.as_tensor(used, device=dm[2].device)
    assert torch.equal(back[dm[2]], got[2])
    assert torch.equal(dm[3][0], got[3][0]) and torch.equal(back[dm[3][1].long()].int(), got[3][1])
    assert torch.equal(dm[3][2], got[3][2])
    assert torch.equal(dm[0].view(torch.int32), got[0].view(torch.int32))
    Gs.close()
    assert sum(dm_classes[:7]) == 0 and sum(dm_classes[8:14]) > 0     # every link ran in a direct-map class


@gpu
@pytest.mark.parametrize("K", [2, 3])
def test_visit_on_a_directed_graph(eng, case, monkeypatch, capfd, K):
    """Every edge of the graph above keeps one direction, a third keep both.  The passes pull over predecessor rows
    (empty ones at hops 2 and 3), every node of S is in P (p == n)."""
    A, links, X = case["A"], case["links"], case["X"]
    coo = A.tocoo()
    up = coo.row < coo.col
    r, c = coo.row[up], coo.col[up]
    rng = np.random.default_rng(14)
    flip = rng.random(len(r)) < 0.5
    both = rng.random(len(r)) < 0.33
    arcs = np.concatenate([np.stack([np.where(flip, c, r), np.where(flip, r, c)], axis=1),
                           np.stack([np.where(flip, r, c), np.where(flip, c, r)], axis=1)[both]])
    Ad = csr_from_arcs(N, arcs)
    A_csc = Ad.tocsc()
    indeg = np.diff(A_csc.indptr)
    for s, d in case["gadget_links"]:
        levels = _hops_of(A, s, d)                 # (the BFS runs on the union of both directions)
        for h in (2, 3):                           # (hop 1 has one or two nodes that could be without a predecessor)
            assert 0 in indeg[levels[h]], (s, d, h)
    G = eng.graph(Ad, directed=True, A_csc=A_csc)
    f, L = eng.features(X), eng.links(links.T.copy())
    for mode, fn in (("pos", oracle.get_PoS_prepped_ds), ("pos_plus", oracle.get_PoS_Plus_prepped_ds)):
        kw = dict(mode=mode, num_hops=HOPS, sign_k=K, directed=True)
        got = plan_outputs(eng, G, L, f, **kw)
        ref, ptr, _ = oracle.collate_rows(fn(links.T, HOPS, Ad, X, 1, KW(K), dtype=np.float64, directed=True,
                                             A_csc=A_csc), K)
        np.testing.assert_array_equal(got[1].cpu().numpy(), ptr)
        err = rel_err(got[0].cpu().numpy(), ref)
        print(f"[link visit] directed {mode} K={K}: rel err {err:.2e}")
        assert err < TOL
        monkeypatch.setenv("S3GRL_DEBUG", "1")
        monkeypatch.setenv("S3GRL_LDS_BUDGET", "400")
        capfd.readouterr()
        scratch = plan_outputs(eng, G, L, f, **kw)
        assert debug_classes(capfd)[-1][6] > 0
        assert_same_outputs(got, scratch)
        monkeypatch.setenv("S3GRL_FORCE_EXT_BITMAPS", "1")
        assert_same_outputs(got, plan_outputs(eng, G, L, f, **kw))
        monkeypatch.delenv("S3GRL_FORCE_EXT_BITMAPS")
        monkeypatch.delenv("S3GRL_LDS_BUDGET")
        monkeypatch.delenv("S3GRL_DEBUG")
    G.close()
