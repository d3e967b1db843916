"""-m gpu: the element plans' gather as two launches (phase A, then the last operator beyond the prefix
as a lean launch that reloads phase A's fp32 partial rows; operands with many entries per row-tile,
like PubMed's) against the chunk path ("packed_only"): bit for bit on the headline list, for jobs that
end inside phase A, for lists gathered in pieces and for folded reversed duplicates; and a link's rows
do not depend on the plan (which other links, in which order) it is gathered in.  Cora PoS Plus (few
entries per row-tile: the one-launch element kernel) is held to the same bits."""
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


def _run(eng, G, X, links, feat, **kw):
    f = eng.features(X, feat)
    assert f.is_packed and not f.is_sparse
    res = eng.precompute(G, f, eng.links(links), **kw)
    f.close()
    return res


def _assert_same(eng, G, X, links, **kw):
    import torch

    a = _run(eng, G, X, links, "auto", **kw)
    b = _run(eng, G, X, links, "packed_only", **kw)
    assert torch.equal(a.row_ptr, b.row_ptr)
    assert torch.equal(a.rows, b.rows)
    return a


@pytest.mark.parametrize("name,mode", [("pubmed_pos_k3", "pos"), ("cora_posplus_k3", "pos_plus")])
def test_split_launch_equals_chunk_path(eng, name, mode):
    from s3grl_amd import workloads

    w = workloads.make(name)
    link_index, _ = w.split.all_links()
    G = eng.graph(w.A)
    res = _assert_same(eng, G, w.X, link_index, mode=mode, num_hops=3, sign_k=3)
    assert res.stats["folded_links"] > 0
    G.close()


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
def test_short_lists_pieces_and_mirrors(eng, monkeypatch, split, mode):
    """Lists from 2 rows (the whole list inside phase A, or a tail of at most three rows after it) to
    the long lists of a random graph, the long ones in pieces when `split`; reversed duplicates and
    repeats of links in the list (folded: the mirror copy is written by the phase-B launch)."""
    g = load_extract("rand300")
    n = int(g["num_nodes"])
    edges = [tuple(e) for e in g["edges"]]
    links = [tuple(l) for l in g["links"][:24]]
    off = n
    for size in range(2, 9):   # disjoint cliques: short lists
        nodes = list(range(off, off + size))
        edges += [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]
        links.append((nodes[0], nodes[-1]))
        off += size
    A = csr_from_undirected(off, np.array(edges))
    rng = np.random.default_rng(11)
    X = (rng.random((off, 530)) * (rng.random((off, 530)) < 0.15)).astype(np.float32)
    links = np.array(links + [l[::-1] for l in links[:8]] + links[:3]).T.copy()
    if split:
        monkeypatch.setenv("S3GRL_SPLIT_T", "48")
        monkeypatch.setenv("S3GRL_SPLIT_SEG_SHIFT", "4")
    G = eng.graph(A)
    res = _assert_same(eng, G, X, links, mode=mode, num_hops=3, sign_k=3)
    assert res.stats["folded_links"] >= 8
    if split:
        assert res.stats["max_nodes"] > 48
    G.close()


def test_link_bits_independent_of_plan(eng):
    """PubMed PoS sign_k 3: every 5th link of 12 000 links of the headline list, in reverse order,
    gathered on its own, gives each of those links the rows it gets among the 12 000."""
    from s3grl_amd import workloads

    w = workloads.make("pubmed_pos_k3")
    link_index, _ = w.split.all_links()
    link_index = np.ascontiguousarray(np.asarray(link_index)[:, :12000])
    sub = np.ascontiguousarray(link_index[:, ::5][:, ::-1])
    G = eng.graph(w.A)
    full = _run(eng, G, w.X, link_index, "auto", mode="pos", num_hops=3, sign_k=3)
    part = _run(eng, G, w.X, sub, "auto", mode="pos", num_hops=3, sign_k=3)
    fp, pp = full.row_ptr.cpu().numpy(), part.row_ptr.cpu().numpy()
    fr, pr = full.rows.cpu().numpy(), part.rows.cpu().numpy()
    L = link_index.shape[1]
    idx = np.arange(0, L, 5)[::-1]
    assert len(idx) == sub.shape[1]
    for j, i in enumerate(idx):
        a = fr[fp[i]:fp[i + 1]]
        b = pr[pp[j]:pp[j + 1]]
        assert a.shape == b.shape
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"link {i}"
    G.close()
