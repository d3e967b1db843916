"""Labelled enclosing subgraphs (SEAL baselines) on the MI355X: s3grl_amd.seal against the reference-pinned
fixtures (labels_*.npz) and the test restatement (tests/seal_reference.py)."""
import numpy as np
import pytest
import scipy.sparse as ssp
import torch

from conftest import GOLDEN, csr_from_arcs, csr_from_undirected
from seal_reference import LABELS, label_subgraph, ragged, tag

pytestmark = pytest.mark.gpu

CASES = ["triangle", "pair", "star_iso", "probe5", "rand300", "usair", "cora", "directed_tiny", "directed_usair"]


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd.engine import Engine

    e = Engine("cuda:0")
    yield e
    e.close()


def run(eng, link_index, A, num_hops, label, x=None, y=1, **kw):
    from s3grl_amd.seal import enclosing_subgraphs

    return enclosing_subgraphs(np.asarray(link_index), A, x, y, num_hops, label, engine=eng, **kw)


def host(subs):
    s = subs.subs
    return {k: getattr(s, k).cpu().numpy() for k in ("node_ptr", "nodes", "dists", "edge_ptr", "src", "dst",
                                                      "weight", "z")}


def link_view(h, i):
    a, b = h["node_ptr"][i], h["node_ptr"][i + 1]
    c, d = h["edge_ptr"][i], h["edge_ptr"][i + 1]
    return (h["nodes"][a:b], h["dists"][a:b], np.stack([h["src"][c:d], h["dst"][c:d], h["weight"][c:d]], 1),
            h["z"][a:b])


def check_against_restatement(h, A, links, labels_of):
    """Every link of `h` equals the restatement on its own node list (edges in the engine's order)."""
    for i in range(len(links)):
        nodes, dists, e, z = link_view(h, i)
        assert nodes[0] == links[i][0] and nodes[1] == links[i][1]
        for label in labels_of:
            edges, zr = label_subgraph(A, nodes, dists, label)
            np.testing.assert_array_equal(e.astype(np.int64), edges, err_msg=f"link {i}")   # same order
            np.testing.assert_array_equal(z, zr, err_msg=f"link {i} {label}")


def load_case(name):
    lab = np.load(GOLDEN / f"labels_{name}.npz")
    ext = np.load(GOLDEN / f"extract_{name}.npz")
    n = int(lab["num_nodes"])
    directed = bool(int(lab["directed"]))
    A = csr_from_arcs(n, lab["arcs"]) if directed else csr_from_undirected(n, lab["edges"])
    return lab, ext, A, directed


@pytest.mark.parametrize("name", CASES)
def test_every_fixture_link_and_label(eng, name):
    lab, ext, A, directed = load_case(name)
    links = lab["links"]
    for hop in (int(x) for x in lab["hops"]):
        for label in LABELS:
            h = host(run(eng, links.T, A, hop, label, directed=directed))
            for i in range(len(links)):
                nodes, dists, e, z = link_view(h, i)
                np.testing.assert_array_equal(nodes, ragged(lab, f"h{hop}_nodes", i))
                np.testing.assert_array_equal(dists, ragged(ext, f"h{hop}_dists", i))
                np.testing.assert_array_equal(z, ragged(lab, f"h{hop}_z_{tag(label)}", i),
                                              err_msg=f"{name} h={hop} link {i} {label}")
                g = np.stack([nodes[e[:, 0].astype(np.int64)], nodes[e[:, 1].astype(np.int64)],
                              e[:, 2].astype(np.int64)], 1)
                g = g[np.lexsort((g[:, 1], g[:, 0]))]
                np.testing.assert_array_equal(g, ragged(lab, f"h{hop}_edges", i).astype(np.int64))


def _split(name):
    from s3grl_amd import workloads as W

    n, e = W.load_topology(name)
    sp = W.edge_split(n, e, seed=0)
    li, _ = sp.all_links()
    return sp.A, li


def test_all_usair_links_two_hops(eng):
    A, li = _split("usair")
    assert li.shape[1] == 7868
    links = li.T
    for label in ("drnl", "de"):
        check_against_restatement(host(run(eng, li, A, 2, label)), A, links, [label])


def test_all_cora_links_three_hops(eng):
    A, li = _split("cora")
    assert li.shape[1] == 19532
    check_against_restatement(host(run(eng, li, A, 3, "drnl")), A, li.T, ["drnl"])


def test_hbm_flavour_is_bit_identical(eng):
    A, li = _split("usair")
    li = li[:, :2000]
    for label in ("drnl", "de", "de+", "degree"):
        a = host(run(eng, li, A, 2, label))
        b = host(run(eng, li, A, 2, label, lds_budget=1))       # nothing fits: every link in HBM
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"{label} {k}")


def test_weighted_graph_edge_weights_and_degree(eng):
    A, li = _split("usair")
    U = ssp.triu(A, k=1).tocoo()                                  # symmetric integer weights 1 .. 4
    w = np.random.default_rng(3).integers(1, 5, size=U.nnz).astype(np.int64)
    W = ssp.coo_matrix((w, (U.row, U.col)), shape=A.shape)
    A = (W + W.T).tocsr()
    li = li[:, :500]
    for label in ("degree", "drnl"):
        subs = run(eng, li, A, 2, label)
        check_against_restatement(host(subs), A, li.T, [label])
        assert subs[0].edge_weight.dtype == torch.int64


def test_star_beyond_65535_nodes(eng):
    leaves = 70000
    edges = np.stack([np.zeros(leaves, np.int64), np.arange(1, leaves + 1)], 1)
    A = csr_from_undirected(leaves + 1, edges)
    links = np.array([[1, 2], [5, 70000]])
    for label in ("drnl", "de", "de+", "degree"):
        h = host(run(eng, links.T, A, 2, label))
        assert h["node_ptr"][1] == leaves + 1
        check_against_restatement(h, A, links, [label])


def test_sampling_uses_the_pos_plan_node_sets(eng):
    A, li = _split("usair")
    li = li[:, :600]
    G = eng.graph(A)
    try:
        plan = eng.plan(G, eng.links(li), mode="pos", num_hops=2, sign_k=1, full_stats=True, fold_reversed=False,
                        ratio_per_hop=0.5, max_nodes_per_hop=20, seed=99)
        node_ptr, nodes, dists = (t.cpu().numpy() for t in plan.export_subgraphs())
        plan.close()
    finally:
        G.close()
    h = host(run(eng, li, A, 2, "de+", ratio_per_hop=0.5, max_nodes_per_hop=20, seed=99))
    np.testing.assert_array_equal(h["node_ptr"], node_ptr)
    np.testing.assert_array_equal(h["dists"], dists)
    for i in range(li.shape[1]):
        a, b = node_ptr[i], node_ptr[i + 1]
        np.testing.assert_array_equal(h["nodes"][a + 2:b], nodes[a + 2:b])
        np.testing.assert_array_equal(np.sort(h["nodes"][a:a + 2]), np.sort(nodes[a:a + 2]))
    check_against_restatement(h, A, li.T, ["de+"])


def test_collate_pyg(eng):
    A, li = _split("usair")
    li = li[:, :300]
    x = torch.randn(A.shape[0], 7)
    subs = run(eng, li, A, 2, "drnl", x=x, y=0)
    batch = subs.collate_pyg()
    h = host(subs)
    xd = x.to(eng.device)
    assert torch.equal(batch.x, xd[batch.node_id])
    assert torch.equal(batch.node_id.cpu(), torch.as_tensor(h["nodes"]).long())
    np.testing.assert_array_equal(batch.batch.cpu().numpy(), np.repeat(np.arange(300), np.diff(h["node_ptr"])))
    link_of_edge = np.repeat(np.arange(300), np.diff(h["edge_ptr"]))
    first = h["node_ptr"][:-1][link_of_edge]
    np.testing.assert_array_equal(batch.edge_index.cpu().numpy(), np.stack([h["src"] + first, h["dst"] + first]))
    assert torch.equal(batch.z.cpu(), torch.as_tensor(h["z"]).long())
    assert batch.y.shape == (300,) and int(batch.y.sum()) == 0
    d = subs[7]
    assert torch.equal(d.x, xd[d.node_id]) and d.num_nodes == d.node_id.numel()
    assert d.edge_index.dtype == torch.int64 and d.z.dtype == torch.int64 and d.y.tolist() == [0]
    none = run(eng, li, A, 2, "drnl", x=None)
    assert none.collate_pyg().x is None and none[0].x is None


def test_edge_cases(eng):
    A, li = _split("usair")
    empty = run(eng, np.zeros((2, 0), np.int64), A, 2, "drnl")
    assert len(empty) == 0 and empty.collate_pyg().edge_index.shape == (2, 0)
    from s3grl_amd.seal import labelled_subgraphs

    G = eng.graph(A)
    try:
        for bad in ([[0, 400]], [[3, 3]], [[-1, 2]]):      # on the device: the C call rejects them
            with pytest.raises(ValueError):
                labelled_subgraphs(eng, G, torch.tensor(bad, device=eng.device), num_hops=2)
    finally:
        G.close()
    li = li[:, :400]
    zeros = host(run(eng, li, A, 2, "cn"))
    assert zeros["z"].shape == zeros["nodes"].shape and not zeros["z"].any()
    for label in ("drnl", "de"):
        a, b = host(run(eng, li, A, 2, label)), host(run(eng, li, A, 2, label))
        for k in a:
            np.testing.assert_array_equal(a[k], b[k])
    fwd = host(run(eng, li, A, 2, "de"))
    rev = host(run(eng, li[::-1].copy(), A, 2, "de"))
    for i in range(li.shape[1]):
        nf, df, ef, zf = link_view(fwd, i)
        nr, dr, er, zr = link_view(rev, i)
        assert nf[0] == nr[1] and nf[1] == nr[0]
        np.testing.assert_array_equal(nf[2:], nr[2:])
        np.testing.assert_array_equal(zf[2:], zr[2:, ::-1])
        np.testing.assert_array_equal(zf[:2], zr[[1, 0]][:, ::-1])
        swap = np.array([1, 0] + list(range(2, len(nf))))
        gf = np.stack([ef[:, 0], ef[:, 1], ef[:, 2]], 1).astype(np.int64)
        gr = np.stack([swap[er[:, 0].astype(np.int64)], swap[er[:, 1].astype(np.int64)], er[:, 2]], 1).astype(np.int64)
        gf = gf[np.lexsort((gf[:, 1], gf[:, 0]))]
        gr = gr[np.lexsort((gr[:, 1], gr[:, 0]))]
        np.testing.assert_array_equal(gf, gr)
