"""-m gpu: the packed gather's last-operator phase on element rows ((column, value) entries, LDS
accumulator) against the same kernel on packed chunks only ("packed_only"): the sums must agree
BIT FOR BIT — the element rows only skip zeros, and every column takes its addends in list order
with the same multiply-adds."""
import numpy as np
import pytest

from conftest import csr_from_undirected, load_extract

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    e = Engine("cuda:0")
    yield e
    e.close()


def _assert_same(eng, G, X, links, modes=("packed", "packed_only"), **kw):
    """rows of the plan through both feature operands; returns the result of the first"""
    import torch

    L = eng.links(links)
    outs = []
    for mode in modes:
        f = eng.features(X, mode)
        assert f.is_packed and not f.is_sparse
        res = eng.precompute(G, f, L, **kw)
        outs.append(res)
        f.close()
    a, b = outs
    assert torch.equal(a.row_ptr, b.row_ptr)
    assert torch.equal(a.rows, b.rows)
    return a


def test_headline_workload(eng):
    """PubMed PoS sign_k 3, 3 hops, all 164 000 links (its biggest lists are gathered in pieces)."""
    from s3grl_amd import workloads

    w = workloads.make("pubmed_pos_k3")
    link_index, _ = w.split.all_links()
    G = eng.graph(w.A)
    res = _assert_same(eng, G, w.X, link_index, modes=("auto", "packed_only"), mode="pos", num_hops=3, sign_k=3)
    assert res.stats["max_nodes"] > 4096 and res.stats["folded_links"] > 30000
    G.close()


def test_cora_pos_plus(eng):
    """Cora PoS Plus sign_k 3, 3 hops, F = 1433 (three column tiles, ~6 entries per row and tile)."""
    from s3grl_amd import workloads

    w = workloads.make("cora_posplus_k3")
    link_index, _ = w.split.all_links()
    G = eng.graph(w.A)
    _assert_same(eng, G, w.X, link_index, modes=("auto", "packed_only"), mode="pos_plus", num_hops=3, sign_k=3)
    G.close()


@pytest.mark.parametrize("F,density", [(7, 0.3), (500, 0.1), (510, 0.4), (1030, 0.05), (1433, 0.0127)])
@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_widths_densities_and_long_rows(eng, F, density, mode, K):
    """F not a multiple of 4 and F > 512; rows with more than 64 (up to 512) entries in a tile; an
    empty row; folded reversed duplicates and repeats in the list; sign_k below the hop count (the
    element phase) and sign_k 1 (the whole list in it)."""
    g = load_extract("rand300")
    n = int(g["num_nodes"])
    A = csr_from_undirected(n, g["edges"])
    rng = np.random.default_rng(F + K)
    X = rng.standard_normal((n, F)) * (rng.random((n, F)) < density)
    X[7] = rng.standard_normal(F)          # fully dense: 512 entries in every full tile
    X[11] = 0                              # empty in every tile
    X[13, ::3] = rng.random((F + 2) // 3) + 0.5   # 171 entries in a full tile
    X = X.astype(np.float32)
    base = g["links"][:16]
    links = np.concatenate([base, base[:6, ::-1], base[:3]]).T.copy()
    G = eng.graph(A)
    res = _assert_same(eng, G, X, links, mode=mode, num_hops=3, sign_k=K)
    assert res.stats["folded_links"] >= 6
    G.close()


@pytest.mark.parametrize("K", [2, 3])
def test_split_jobs(eng, monkeypatch, K):
    """Lists gathered in pieces (partial rows combined afterwards) take the same path."""
    g = load_extract("rand300")
    n = int(g["num_nodes"])
    A = csr_from_undirected(n, g["edges"])
    rng = np.random.default_rng(5 + K)
    X = (rng.random((n, 300)) * (rng.random((n, 300)) < 0.2)).astype(np.float32)
    links = g["links"][:20].T.copy()
    G = eng.graph(A)
    monkeypatch.setenv("S3GRL_SPLIT_T", "48")
    monkeypatch.setenv("S3GRL_SPLIT_SEG_SHIFT", "4")
    res = _assert_same(eng, G, X, links, mode="pos", num_hops=3, sign_k=K)
    assert res.stats["max_nodes"] > 48
    G.close()


@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
def test_tiny_supports(eng, mode):
    """Disjoint cliques of 2..7 nodes: every list is 2-7 rows long (no full group of four, or one
    group and a tail)."""
    edges, links, off = [], [], 0
    for size in range(2, 8):
        for rep in range(3):
            nodes = list(range(off, off + size))
            edges += [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]
            links.append((nodes[0], nodes[-1]))
            off += size
    n = off
    A = csr_from_undirected(n, np.array(edges))
    rng = np.random.default_rng(3)
    X = (rng.random((n, 600)) * (rng.random((n, 600)) < 0.1)).astype(np.float32)
    G = eng.graph(A)
    for K in (1, 2):
        _assert_same(eng, G, X, np.array(links).T.copy(), mode=mode, num_hops=3, sign_k=K)
    G.close()
