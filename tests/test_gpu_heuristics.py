"""Link heuristics on the MI355X (s3grl_amd.heuristics, csrc/s3grl_heuristics.hip) against the fp64 restatement
(tests/heuristics_reference.py): CN bit-equal and AA within rtol 1e-6 on real val/test lists and on edge cases,
PPR scores and per-source iteration counts, determinism across runs, block widths and source orders, and the
Table 2 row of run_heuristic."""
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import heuristics_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"


def _split(name):
    from s3grl_amd import workloads as W

    if name == "router":
        n, e = W.read_seal_edges(GOLDEN / "router_edges.txt")
        e = W.undirected_unique(e)
    else:
        n, e = W.load_topology(name)
    return W.edge_split(n, e, seed=0)


def _val_test(sp):
    return np.concatenate([sp.links["valid"][0], sp.links["valid"][1], sp.links["test"][0], sp.links["test"][1]],
                          axis=1)


def _heur(A):
    from s3grl_amd.heuristics import Heuristics

    return Heuristics(A)


def _edge_case_links(A, rng, count=3000):
    """random pairs plus hubs, isolated nodes, s == d and duplicated links"""
    n = A.shape[0]
    deg = np.diff(A.indptr)
    hubs = np.argsort(-deg)[:5]
    iso = np.nonzero(deg == 0)[0][:5]
    s = rng.integers(0, n, count)
    d = rng.integers(0, n, count)
    extra = [np.stack([np.repeat(hubs, len(hubs)), np.tile(hubs, len(hubs))]),
             np.stack([hubs, rng.integers(0, n, len(hubs))]), np.stack([s[:50], s[:50]])]
    if len(iso):
        extra += [np.stack([iso, hubs[:len(iso)]]), np.stack([rng.integers(0, n, len(iso)), iso])]
    L = np.concatenate([np.stack([s, d])] + extra, axis=1)
    return np.concatenate([L, L[:, :200]], axis=1)


@pytest.mark.parametrize("name", ["usair", "router", "cora"])
def test_cn_aa_on_val_test_lists(name):
    sp = _split(name)
    h = _heur(sp.A)
    rng = np.random.default_rng(1)
    for links in (_val_test(sp), _edge_case_links(sp.A, rng)):
        cn = h.cn(torch.as_tensor(links)).cpu().numpy()
        aa = h.aa(links).cpu().numpy()
        assert cn.dtype == np.float32 and cn.shape == (links.shape[1],)
        assert np.array_equal(cn, R.cn(sp.A, links))
        np.testing.assert_allclose(aa, R.aa(sp.A, links), rtol=1e-6, atol=0)
        sw = links[::-1].copy()                                     # (d, s) takes the same path
        assert np.array_equal(h.aa(sw).cpu().numpy(), aa)
    h.close()


def test_cn_aa_weighted_graphs():
    rng = np.random.default_rng(2)
    n, m = 400, 3000
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    links = _edge_case_links(ssp.csr_matrix((np.ones(m), (r, c)), shape=(n, n)), rng, 2000)
    ints = rng.integers(1, 6, m).astype(np.int64)                  # int weights > 1, duplicates summed
    A = ssp.csr_matrix((np.r_[ints, ints], (np.r_[r, c], np.r_[c, r])), shape=(n, n))
    h = _heur(A)
    assert np.array_equal(h.cn(links).cpu().numpy(), R.cn(A, links))
    np.testing.assert_allclose(h.aa(links).cpu().numpy(), R.aa(A, links), rtol=1e-6)
    h.close()
    fl = rng.random(m) * 1.5 + 0.05                                 # float weights, column sums below 1 too
    A = ssp.csr_matrix((fl, (r, c)), shape=(n, n))                  # directed
    h = _heur(A)
    np.testing.assert_allclose(h.cn(links).cpu().numpy(), R.cn(A, links), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(h.aa(links).cpu().numpy(), R.aa(A, links), rtol=1e-6, atol=1e-6)
    h.close()


def _check_ppr(A, links, got, its):
    ref, ref_its = R.ppr_scores(A, links)
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-12)
    src, first = np.unique(links[0], return_index=True)
    a, b = its[first], ref_its[first]
    assert np.abs(a - b).max() <= 1
    assert np.mean(a == b) >= 0.99, f"{np.mean(a == b):.4f} of {len(src)} sources stop at the same iteration"


def test_ppr_usair_all_val_test_links():
    sp = _split("usair")
    links = _val_test(sp)
    h = _heur(sp.A)
    got, its = h.ppr(links, return_iterations=True)
    _check_ppr(sp.A, links, got.cpu().numpy(), its.cpu().numpy())
    h.close()


@pytest.mark.parametrize("name", ["router", "pubmed"])
def test_ppr_sampled_sources(name):
    sp = _split(name)
    links = _val_test(sp)
    rng = np.random.default_rng(3)
    src = rng.choice(np.unique(links[0]), 256, replace=False)
    links = links[:, np.isin(links[0], src)]
    h = _heur(sp.A)
    got, its = h.ppr(links, return_iterations=True)
    _check_ppr(sp.A, links, got.cpu().numpy(), its.cpu().numpy())
    h.close()


def test_ppr_deterministic_across_runs_widths_and_orders():
    sp = _split("cora")
    links = _val_test(sp)
    h = _heur(sp.A)
    a = h.ppr(links).cpu().numpy()
    assert np.array_equal(a, h.ppr(links).cpu().numpy())
    b, ib = h.ppr(links, block_width=64, return_iterations=True)
    assert np.array_equal(a, b.cpu().numpy())
    rng = np.random.default_rng(4)
    perm = rng.permutation(links.shape[1])
    dup = np.concatenate([links[:, perm], links[:, perm[:500]]], axis=1)
    c, ic = h.ppr(dup, block_width=128, return_iterations=True)
    assert np.array_equal(c.cpu().numpy()[:len(perm)], a[perm])
    assert np.array_equal(c.cpu().numpy()[len(perm):], a[perm[:500]])
    assert np.array_equal(ic.cpu().numpy()[:len(perm)], ib.cpu().numpy()[perm])
    # a few sources alone in their block give the same bits as inside a full one
    few = links[:, np.isin(links[0], np.unique(links[0])[:3])]
    assert np.array_equal(h.ppr(few).cpu().numpy(), a[np.isin(links[0], np.unique(links[0])[:3])])
    h.close()


def test_ppr_isolated_source_and_small_graph():
    # node 5 is isolated: one iteration, all mass on itself
    r, c, v = [0, 1, 2, 2, 3], [1, 2, 0, 3, 4], [1.0, 2.0, 3.0, 0.5, 1.0]
    A = ssp.csr_matrix((v + v, (r + c, c + r)), shape=(6, 6))
    links = np.array([[5, 5, 0, 0, 3], [5, 1, 4, 0, 3]])
    h = _heur(A)
    got, its = h.ppr(links, return_iterations=True)
    got, its = got.cpu().numpy(), its.cpu().numpy()
    assert got[0] == 1.0 and got[1] == 0.0 and its[0] == 1
    _check_ppr(A, links, got, its)
    conv = h.ppr(links, tol=1e-12, max_iter=10000).cpu().numpy()
    ref = np.array([R.ppr_dense(A, s)[d] for s, d in links.T])
    np.testing.assert_allclose(conv, ref, rtol=1e-5, atol=1e-7)
    h.close()


def test_empty_and_bad_inputs():
    from s3grl_amd import heuristics as H

    sp = _split("usair")
    h = _heur(sp.A)
    e = np.zeros((2, 0), dtype=np.int64)
    for fn in (h.cn, h.aa, h.ppr):
        out = fn(e)
        assert out.shape == (0,) and out.is_cuda
    with pytest.raises(ValueError):
        h.cn(np.array([[0], [sp.num_nodes]]))
    with pytest.raises(ValueError):
        h.ppr(np.array([[-1], [0]]))
    with pytest.raises(ValueError):
        h.ppr(_val_test(sp), block_width=96)
    h.close()
    s, ei = H.PPR(sp.A, torch.as_tensor(_val_test(sp)))
    assert s.device.type == "cpu" and np.all(np.diff(ei[0].numpy()) >= 0)
    s2, ei2 = H.CN(sp.A, _val_test(sp))
    assert s2.dtype == torch.float32 and s2.shape == (ei2.shape[1],)


def test_run_heuristic_usair_matches_restatement():
    from s3grl_amd.heuristics import evaluate_auc, run_heuristic

    sp = _split("usair")
    lists = [sp.links["valid"][0], sp.links["valid"][1], sp.links["test"][0], sp.links["test"][1]]
    fns = {"CN": R.cn, "AA": R.aa, "PPR": lambda A, L: R.ppr_scores(A, L)[0]}
    for name, fn in fns.items():
        sc = [fn(sp.A, L) for L in lists]
        want = evaluate_auc(np.r_[sc[0], sc[1]], np.r_[np.ones(len(sc[0])), np.zeros(len(sc[1]))],
                            np.r_[sc[2], sc[3]], np.r_[np.ones(len(sc[2])), np.zeros(len(sc[3]))])
        got = run_heuristic(sp, name)
        for k in ("AUC", "AP"):
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-6), (name, k, got[k], want[k])
        assert got["AUC"][1] > 0.8, (name, got)
