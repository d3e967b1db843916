"""SoP links whose scalar ball does not fit a CU's LDS (class 3): the ball's node list and propagated rows
live in an HBM workspace slice per workgroup.  Host tests of `engine.sop_layout` (no GPU) and GPU tests of
parity, orientation, chunking and flavour independence.  Bar: `rel_err` of tests/test_gpu_parity.py
(row-norm floored, ATOL 1e-10) below 1e-5, on every link of every list.

The oracle's explicit powers Â^i are dense for a star, so the big graphs are checked against
`sop_rows_sparse`: row s of Â^i by i sparse vector-matrix products in fp64 — which a CPU test pins to the
oracle on a fixture first."""
import numpy as np
import pytest

import oracle
from conftest import csr_from_undirected, load_extract

TOL = 1e-5
ATOL = 1e-10
gpu = pytest.mark.gpu


def rel_err(got, ref):
    """tests/test_gpu_parity.py's: max over elements of (|got - ref| - ATOL)+ / max(|ref|, ‖ref row‖∞)"""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=-1, keepdims=True))
    return float(np.max(np.clip(np.abs(got - ref) - ATOL, 0, None) / np.maximum(scale, 1e-30)))


def sop_rows_sparse(A, X, links, K):
    """rows [2L, K+1, 1+F] of the SoP flow in fp64 without a power of Â: row a of Â^i is i vector-matrix
    products from e_a; column b (the other endpoint) is zeroed, the row multiplied by X and Â^i[a,a]
    prepended.  links [2, L]."""
    op = oracle.global_normalized_powers(A, 1, np.float64)[0].tocsr()
    opT = op.T.tocsr()
    X = np.asarray(X, dtype=np.float64)
    n, F = X.shape
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    L = links.shape[1]
    cache = {}

    def power_rows(a):
        if a not in cache:
            v = np.zeros(n)
            v[a] = 1.0
            out = []
            for _ in range(K):
                v = opT @ v          # (e_aᵀ Â^i)ᵀ = Âᵀ (e_aᵀ Â^{i-1})ᵀ
                out.append(v)
            cache[a] = out
        return cache[a]

    rows = np.empty((2 * L, K + 1, 1 + F))
    for l in range(L):
        s, d = int(links[0, l]), int(links[1, l])
        for e, (a, b) in enumerate(((s, d), (d, s))):
            rows[2 * l + e, 0, 0] = 1.0
            rows[2 * l + e, 0, 1:] = X[a]
            for i, v in enumerate(power_rows(a)):
                w = v.copy()
                w[b] = 0.0
                rows[2 * l + e, i + 1, 0] = v[a]
                rows[2 * l + e, i + 1, 1:] = w @ X
    return rows


# ------------------------------------------------------------------------------------------------------
# host
# ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6])
def test_sparse_reference_equals_the_oracle(K):
    g = load_extract("rand300")
    n = int(g["num_nodes"])
    A = csr_from_undirected(n, g["edges"])
    X = np.random.default_rng(K).standard_normal((n, 11))
    links = g["links"].T
    ref, _, _ = oracle.collate_rows(
        oracle.get_SoP_prepped_ds(oracle.global_normalized_powers(A, K, np.float64), links, A, X, 1,
                                  dtype=np.float64), K)
    mine = sop_rows_sparse(A, X, links, K)
    assert mine.shape == ref.shape
    assert np.max(np.abs(mine - ref)) <= 1e-12      # every link, every operator, both endpoints


@pytest.mark.parametrize("n,K,nodes,ext", [(235000, 3, 2053, False), (19717, 3, 4295, False), (19717, 8, 2274, False),
                                           (6000, 3, 4438, False), (400000, 3, 4501, True)])
def test_sop_layout_nodes_that_fit_lds(n, K, nodes, ext):
    from s3grl_amd import engine

    lay = engine.sop_layout(n, K)
    hb = (K + 1) // 2
    assert lay["nodes_lds"] == nodes and lay["external_bitmaps"] is ext
    assert lay["bytes_per_node"] == 4 + 16 * hb
    # the issue's formula
    w_lds = 0 if ext else (n + 31) // 32
    fixed = 4 * (3 * w_lds + 32 + 32 + 256 + 96) + 64
    assert lay["fixed_lds_bytes"] == fixed
    assert lay["nodes_lds"] == (163840 - fixed - 64) // (4 + 16 * hb)
    c0, c1, c2 = lay["class_nodes"]
    assert c0 <= c1 <= c2 == lay["nodes_lds"]
    assert c0 == (min(12288, 163840 - fixed) - 64) // lay["bytes_per_node"]
    assert c1 == (min(49152, 163840 - fixed) - 64) // lay["bytes_per_node"]


def test_sop_layout_radius_and_arguments():
    from s3grl_amd import engine

    assert [engine.sop_layout(1000, K)["radius"] for K in range(1, 9)] == [0, 1, 1, 2, 2, 3, 3, 4]
    for bad in [(0, 3), (1000, 0), (1000, 9)]:
        with pytest.raises(ValueError):
            engine.sop_layout(*bad)


# ------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    e = Engine("cuda:0")
    yield e
    e.close()


N_DS = 6000


@pytest.fixture(scope="module")
def double_star():
    """Hub 0 with leaves 2..2601, hub 1 with leaves 2602..5201, the edge (0,1), and 3000 random edges among
    nodes 1000..5999.  deg 0 = deg 1 = 2601: the 1-hop bound of (0,1) is 5204 against 4438 nodes of LDS."""
    rng = np.random.default_rng(7)
    e = rng.integers(1000, N_DS, size=(4000, 2))
    e = e[e[:, 0] != e[:, 1]]
    e = np.unique(np.sort(e, axis=1), axis=0)
    e = e[rng.permutation(len(e))[:3000]]
    assert len(e) == 3000
    star0 = np.stack([np.zeros(2600, dtype=np.int64), np.arange(2, 2602)], axis=1)
    star1 = np.stack([np.ones(2600, dtype=np.int64), np.arange(2602, 5202)], axis=1)
    edges = np.concatenate([star0, star1, [[0, 1]], e])
    A = csr_from_undirected(N_DS, edges)
    assert A.max() == 1 and A[0].nnz == 2601 and A[1].nnz == 2601
    X = np.random.default_rng(8).standard_normal((N_DS, 9)).astype(np.float32)
    links = np.array([[0, 1], [1, 0], [0, 2700], [5, 0], [5, 2700], [1500, 4000], [5500, 5800], [0, 1]])
    links = links[np.random.default_rng(9).permutation(len(links))].T.copy()
    return A, X, links


_REFS = {}


def ds_reference(double_star, K):
    """computed once per K, shared, never written to"""
    if K not in _REFS:
        A, X, links = double_star
        ref = sop_rows_sparse(A, X.astype(np.float64), links, K)
        ref.setflags(write=False)
        _REFS[K] = ref
    return _REFS[K]


def run_sop(eng, A, X, links, K):
    """-> (rows [2L, K+1, 1+F] torch, class counts)"""
    from s3grl_amd.engine import Sop

    G = eng.graph(A)
    sop = Sop(eng, G, eng.features(X), K)
    try:
        rows = sop.run(eng.links(links)).clone()
        cls = tuple(sop.last_class_links)
    finally:
        sop.close()
        G.close()
    return rows, cls


@gpu
@pytest.mark.parametrize("K", [3, 4, 5, 8])
def test_double_star_parity_and_orientation(eng, double_star, K):
    import torch

    A, X, links = double_star
    rows, cls = run_sop(eng, A, X, links, K)
    ref = ds_reference(double_star, K)
    got = rows.cpu().numpy()
    for l in range(links.shape[1]):           # every link, named when it fails
        err = rel_err(got[2 * l:2 * l + 2], ref[2 * l:2 * l + 2])
        assert err < TOL, (tuple(links[:, l]), err)
    assert cls[3] > 0
    if K == 3:
        assert cls[0] > 0
    pairs = [tuple(p) for p in links.T.tolist()]
    fwd, rev = pairs.index((0, 1)), pairs.index((1, 0))
    dup = len(pairs) - 1 - pairs[::-1].index((0, 1))
    assert dup != fwd
    # (d,s) has the rows of (s,d) swapped, and an exact duplicate the same rows, bit for bit
    assert torch.equal(rows[2 * rev], rows[2 * fwd + 1]) and torch.equal(rows[2 * rev + 1], rows[2 * fwd])
    assert torch.equal(rows[2 * dup:2 * dup + 2], rows[2 * fwd:2 * fwd + 2])


@gpu
def test_star_leaf_rows_cancel_exactly_in_an_hbm_ball(eng):
    """Star with 4600 leaves, link (leaf, hub), sign_k = 5: the 2-hop ball is the whole graph, 4601 nodes
    against 3083 of LDS (52 bytes per node at sign_k 5), so the link is class 3.  Every odd power of Â sends
    the leaf to the hub only: its masked row is exactly zero in the reference."""
    from s3grl_amd import engine

    n = 4601
    assert engine.sop_layout(n, 5)["nodes_lds"] < n
    A = csr_from_undirected(n, np.stack([np.zeros(n - 1, dtype=np.int64), np.arange(1, n)], axis=1))
    X = np.random.default_rng(0).standard_normal((n, 9)).astype(np.float32)
    links = np.array([[3], [0]])
    rows, cls = run_sop(eng, A, X, links, 5)
    assert cls == (0, 0, 0, 1)
    rows = rows.cpu().numpy()
    ref = sop_rows_sparse(A, X.astype(np.float64), links, 5)
    for i in (1, 3, 5):
        assert np.all(np.abs(ref[0, i, 1:]) < 1e-15)
        assert np.all(np.abs(rows[0, i, 1:]) < 1e-12)
    assert rel_err(rows, ref) < TOL


@gpu
@pytest.mark.parametrize("name", ["rand300", "usair"])
@pytest.mark.parametrize("K", [1, 2, 3, 6])
def test_flavour_changes_no_bit(eng, monkeypatch, name, K):
    """S3GRL_SOP_FORCE_HBM_BALLS sends every link of a small fixture through the HBM flavour: the same rows,
    bit for bit, also with the bitmaps in HBM slices and with reversed duplicates not folded."""
    import torch

    g = load_extract(name)
    n = int(g["num_nodes"])
    A = csr_from_undirected(n, g["edges"])
    X = np.random.default_rng(20 + K).standard_normal((n, 13)).astype(np.float32)
    base = g["links"]
    links = np.concatenate([base, base[::2, ::-1], base[:5]])       # reversed duplicates, exact duplicates
    links = links[np.random.default_rng(K).permutation(len(links))].T.copy()
    plain, cls = run_sop(eng, A, X, links, K)
    assert cls[3] == 0 and sum(cls) > 0
    ref, _, _ = oracle.collate_rows(
        oracle.get_SoP_prepped_ds(oracle.global_normalized_powers(A, K, np.float64), links, A,
                                  X.astype(np.float64), 1, dtype=np.float64), K)
    assert rel_err(plain.cpu().numpy(), ref) < TOL
    monkeypatch.setenv("S3GRL_SOP_FORCE_HBM_BALLS", "1")
    forced, fcls = run_sop(eng, A, X, links, K)
    assert fcls == (0, 0, 0, sum(cls))
    assert torch.equal(forced, plain)
    monkeypatch.setenv("S3GRL_FORCE_EXT_BITMAPS", "1")
    assert torch.equal(run_sop(eng, A, X, links, K)[0], plain)
    monkeypatch.delenv("S3GRL_FORCE_EXT_BITMAPS")
    monkeypatch.setenv("S3GRL_NO_MIRROR", "1")
    assert torch.equal(run_sop(eng, A, X, links, K)[0], plain)


@gpu
def test_chunked_workspace_changes_no_bit(eng, monkeypatch, double_star):
    """sign_k = 4 on the double star: every class-3 ball holds both stars (5202 nodes or more, the whole
    graph at most), so a slice takes 187 272 .. 216 000 bytes (36 per node).  A cap of 432 000 bytes holds two
    slices and never three: an odd number n3 >= 5 of class-3 links runs in (n3 + 1) / 2 >= 3 chunks, the last one
    a single link.  (The list has an even number of them: one more hub link is appended.)  A cap below one
    slice runs one link per chunk."""
    import torch

    A, X, links = double_star
    K = 4
    _, cls = run_sop(eng, A, X, links, K)
    if cls[3] % 2 == 0:
        links = np.concatenate([links, [[1], [7]]], axis=1)
    plain, cls = run_sop(eng, A, X, links, K)
    assert cls[3] >= 5 and cls[3] % 2 == 1
    ref = sop_rows_sparse(A, X.astype(np.float64), links, K)
    assert rel_err(plain.cpu().numpy(), ref) < TOL
    for cap in (432000, 1000):
        monkeypatch.setenv("S3GRL_SOP_BALL_WORKSPACE_BYTES", str(cap))
        rows, ccls = run_sop(eng, A, X, links, K)
        assert ccls == cls
        assert torch.equal(rows, plain), cap


@gpu
def test_dropin_and_hybrid_on_the_double_star(eng, double_star):
    import torch
    from s3grl_amd.tuned_SIGN import OptimizedSignOperations, clear_cache

    A, X, links = double_star
    L = links.shape[1]
    ref = ds_reference(double_star, 3)
    lst = OptimizedSignOperations.get_SoP_prepped_ds([None] * 3, torch.from_numpy(links), A, torch.from_numpy(X), 1)
    assert len(lst) == L and lst[0].y == 1
    for l, d in enumerate(lst):
        for i, k in enumerate(("x", "x1", "x2", "x3")):
            assert d[k].shape == (2, 10)
            assert rel_err(d[k].numpy(), ref[2 * l:2 * l + 2, i]) < TOL, (l, k)
    clear_cache()
    G = eng.graph(A)
    res = eng.precompute(G, eng.features(X), eng.links(links), mode="hybrid", num_hops=1, sign_k=3)
    rows = res.rows.cpu().numpy()
    # reference utils.py:454-480: the PoS operators, then SoP's x2..xK
    assert rows.shape == (2 * L, 4 + 2, 10)
    np.testing.assert_array_equal(res.row_ptr.cpu().numpy(), np.arange(0, 2 * L + 1, 2))
    assert rel_err(rows[:, 4:], ref[:, 2:]) < TOL
    pos = eng.precompute(G, eng.features(X), eng.links(links), mode="pos", num_hops=1, sign_k=3)
    assert torch.equal(res.rows[:, :4], pos.rows)
    G.close()
