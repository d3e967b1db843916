"""CPU checks of the link heuristics: the fp64 restatement (tests/heuristics_reference.py) against itself (batched PPR
against the literal per-source loop), against the converged linear-system answer and against hand-computed CN / AA;
the numpy AUC / AP of s3grl_amd.heuristics against sklearn; and the argument checks that refuse before any GPU
work."""
import math

import numpy as np
import pytest
import scipy.sparse as ssp

import heuristics_reference as R


def _usair_split():
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    return W.edge_split(n, e, seed=0)


def _val_test_links(sp):
    return np.concatenate([sp.links["valid"][0], sp.links["valid"][1], sp.links["test"][0], sp.links["test"][1]],
                          axis=1)


def test_batched_ppr_equals_the_per_source_loop_on_usair():
    sp = _usair_split()
    src = np.unique(_val_test_links(sp)[0])
    loop = R.ppr_loop(sp.A, src)
    X, its = R.ppr_batched(sp.A, src)
    assert np.array_equal(its, np.array([loop[int(s)][1] for s in src]))
    ref = np.stack([loop[int(s)][0] for s in src], axis=1)
    assert np.allclose(X, ref, rtol=1e-12, atol=0)
    assert its.min() >= 1 and its.max() <= 100
    assert np.median(its) < 100                 # many columns stop before max_iter


def test_converged_ppr_matches_the_linear_system():
    # 6 nodes: a weighted triangle with a tail, a weight below 1, and node 5 isolated
    r = [0, 1, 2, 2, 3]
    c = [1, 2, 0, 3, 4]
    v = [1.0, 2.0, 3.0, 0.5, 1.0]
    A = ssp.csr_matrix((v + v, (r + c, c + r)), shape=(6, 6))
    for s in range(6):
        x, it = R.pagerank_power(A, s, tol=1e-14, max_iter=10000)
        assert it < 10000
        assert np.allclose(x, R.ppr_dense(A, s), rtol=1e-10, atol=1e-13)
    x, it = R.pagerank_power(A, 5)
    assert it == 1 and x[5] == 1.0 and np.count_nonzero(x) == 1
    X, its = R.ppr_batched(A, np.arange(6), tol=1e-14, max_iter=10000)
    for s in range(6):
        assert np.allclose(X[:, s], R.ppr_dense(A, s), rtol=1e-10, atol=1e-13)
    assert its[5] == 1


def test_cn_and_aa_by_hand():
    # a path 0-1-2 plus 0-3 (weight 2), 3-2 (weight 0.5), node 4 hangs off 3 only, node 5 isolated
    und = [(0, 1, 1.0), (1, 2, 1.0), (0, 3, 2.0), (3, 2, 0.5), (3, 4, 1.0)]
    r = [a for a, b, _ in und] + [b for a, b, _ in und]
    c = [b for a, b, _ in und] + [a for a, b, _ in und]
    v = [w for *_, w in und] * 2
    A = ssp.csr_matrix((v, (r, c)), shape=(6, 6))
    colsum = np.asarray(A.sum(axis=0)).ravel()   # 3, 2, 1.5, 3.5, 1, 0
    assert np.allclose(colsum, [3, 2, 1.5, 3.5, 1, 0])
    links = np.array([[0, 0, 2, 4, 5, 1], [2, 4, 4, 3, 0, 1]])
    # CN(0,2) = A01·A21 + A03·A23 = 1 + 2·0.5; CN(0,4) = A03·A43 = 2; CN(2,4) = A23·A43 = 0.5; CN(4,3) = 0;
    # isolated 5: 0; CN(1,1) = A10² + A12² = 2
    assert np.array_equal(R.cn(A, links), np.float32([2.0, 2.0, 0.5, 0.0, 0.0, 2.0]))
    w = R.aa_weights(A)
    assert w[4] == 0.0                             # c = 1: 1/ln 1 = inf -> 0
    assert math.copysign(1.0, w[5]) == -1.0 and w[5] == 0.0   # c = 0: -0.0
    assert np.isclose(w[2], 1 / math.log(1.5)) and w[2] > 0
    expect = [1 * 1 * w[1] + 2 * 0.5 * w[3], 2 * 1 * w[3], 0.5 * 1 * w[3], 0.0, 0.0, w[0] + w[2]]
    assert np.allclose(R.aa(A, links), np.float32(expect), rtol=1e-6)
    # a column sum in (0, 1): its weight is negative and kept
    B = ssp.csr_matrix(([0.5, 0.5, 0.25, 0.25], ([0, 1, 2, 1], [1, 0, 1, 2])), shape=(3, 3))
    wb = R.aa_weights(B)
    assert wb[0] < 0 and wb[2] < 0
    assert R.aa(B, np.array([[0], [2]]))[0] == np.float32(0.5 * 0.25 * wb[1])


def test_evaluate_auc_equals_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    from s3grl_amd.heuristics import evaluate_auc

    rng = np.random.default_rng(0)
    for tied in (False, True):
        yv, yt = rng.integers(0, 2, 301), rng.integers(0, 2, 250)
        pv, pt = rng.random(301), rng.random(250)
        if tied:
            pv, pt = np.round(pv * 5), np.round(pt * 3)     # many ties, as integer CN scores have
        got = evaluate_auc(pv, yv, pt, yt)
        want = {"AUC": (metrics.roc_auc_score(yv, pv), metrics.roc_auc_score(yt, pt)),
                "AP": (metrics.average_precision_score(yv, pv), metrics.average_precision_score(yt, pt))}
        for k in ("AUC", "AP"):
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-12), (k, tied, got[k], want[k])


def test_bad_ids_raise_before_any_gpu_work():
    from s3grl_amd import heuristics as H

    A = ssp.csr_matrix(([1, 1], ([0, 1], [1, 0])), shape=(3, 3))
    for bad in ([[0, 3], [1, 0]], [[0, -1], [1, 2]], [[0, 1, 2]]):
        ei = np.array(bad)
        for fn in (H.CN, H.AA, H.PPR):
            with pytest.raises(ValueError):
                fn(A, ei)
    with pytest.raises(ValueError):
        H.check_links(np.array([[0.5], [1.0]]), 3)
    assert H.check_links(np.zeros((2, 0), dtype=np.int64), 3).shape == (2, 0)


def test_importing_heuristics_leaves_tuned_sign_alone():
    import os
    import subprocess
    import sys

    code = ("import sys, s3grl_amd.heuristics, s3grl_amd; s3grl_amd.Heuristics; "
            "assert 's3grl_amd.tuned_SIGN' not in sys.modules; print('ok')")
    from pathlib import Path

    r = subprocess.run([sys.executable, "-c", code], cwd=str(Path(__file__).resolve().parent.parent),
                       capture_output=True, text=True, env=dict(os.environ))
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


# ---- the builders of tests/heuristics_cases.py deliver what tests/test_gpu_heuristics_shapes.py relies on ----

def _walked_searched(c, s, d):
    """the rows pairs_kernel walks and searches for the link (s, d): the shorter is walked, a tie walks the
    smaller id"""
    ls, ld = len(c.rows[s]), len(c.rows[d])
    walk_s = ls < ld or (ls == ld and s <= d)
    return (c.rows[s], c.rows[d]) if walk_s else (c.rows[d], c.rows[s])


def test_comb_graph_has_every_length_pair_and_overlap_pattern():
    import heuristics_cases as K

    c = K.comb_graph()
    assert c.A_int.shape == (700, 700) and c.links.shape[1] == len(c.cases)
    for A in (c.A_int, c.A_float, c.A_signed):
        assert A.has_sorted_indices and np.all(A.data != 0)
        assert np.array_equal(A.indptr, c.A_int.indptr) and np.array_equal(A.indices, c.A_int.indices)
    length = np.diff(c.A_int.indptr)
    assert all(np.array_equal(c.A_int.indices[c.A_int.indptr[i]:c.A_int.indptr[i + 1]], r)
               for i, r in enumerate(c.rows))
    pairs = {(int(length[s]), int(length[d])) for s, d in c.links.T}
    assert {(a, b) for a in K.LENGTHS for b in K.LENGTHS} <= pairs
    assert {int(length[s]) for s, d in c.links.T if s == d} == set(K.LENGTHS)
    seen = {p: set() for p in K.PATTERNS}
    tie_orders = {p: set() for p in K.PATTERNS}
    for s, d, a, b, pattern in c.cases:
        assert (length[s], length[d]) == (a, b)
        if pattern is None:
            continue
        W, S = _walked_searched(c, s, d)
        both = np.intersect1d(W, S)
        if pattern == "disjoint":
            assert len(both) == 0
        elif pattern == "identical":
            assert np.array_equal(W, S)
        elif pattern == "first":
            assert np.array_equal(both, S[:1]) and (len(W) < 2 or S[0] - 1 in W)
        elif pattern == "last":
            assert np.array_equal(both, S[-1:]) and (len(W) < 2 or S[-1] + 1 in W)
        elif pattern == "below":
            assert W.max() == S[0] - 1
        else:
            assert pattern == "above" and W.min() == S[-1] + 1
        seen[pattern].add((len(W), len(S)))
        if a == b:
            tie_orders[pattern].add(bool(s < d))       # equal lengths: the link in both orders
    for p in K.PATTERNS:
        assert len(seen[p]) >= 6, (p, seen[p])
        assert tie_orders[p] == {True, False}
        assert seen[p] >= {(64, 64), (128, 128), (200, 200)}
    for L, at in c.cuts.items():
        assert len(at) == L and np.all(R.cn(c.A_int, c.links[:, at]) > 0)
    assert sorted(c.cuts) == [1, 3, 4, 5]


def test_comb_value_sets_and_signed_column_sums():
    import heuristics_cases as K

    c = K.comb_graph()
    assert set(np.unique(c.A_int.data)) == {1.0, 2.0, 3.0, 4.0, 5.0}
    assert c.A_float.data.min() >= 0.05 and c.A_float.data.max() < 1.55
    cs = np.asarray(c.A_signed.sum(axis=0)).ravel()
    assert np.all(cs[c.columns["zero"]] == 0.0) and np.all(cs[c.columns["one"]] == 1.0)
    assert np.all((cs[c.columns["half"]] > 0) & (cs[c.columns["half"]] < 1)) and np.all(cs[c.columns["negative"]] < 0)
    assert np.mean(np.abs(c.A_signed.data) == 1.0) > 0.99 and (c.A_signed.data < 0).mean() > 0.2
    with np.errstate(divide="ignore", invalid="ignore"):
        w = R.aa_weights(c.A_signed)
        aa = R.aa(c.A_signed, c.links)
    assert np.all(w[c.columns["one"]] == 0.0) and not np.signbit(w[c.columns["one"]]).any()
    assert np.all(w[c.columns["zero"]] == 0.0) and np.signbit(w[c.columns["zero"]]).all()
    assert np.all(w[c.columns["half"]] < 0) and np.isnan(w[c.columns["negative"]]).all()
    # every special column is a common key of some link, and the scores hold NaN, zero and finite values
    for which, ks in c.columns.items():
        for k in ks:
            assert any(k in c.rows[s] and k in c.rows[d] for s, d in c.links.T), (which, k)
    assert 10 <= np.isnan(aa).sum() <= 0.4 * len(aa) and np.count_nonzero(np.nan_to_num(aa)) >= 50
    # the reference's sparse product keeps 0·NaN: a NaN-weighted key in row d alone gives NaN, in row s alone not
    nan_row = np.array([np.isnan(w[r]).any() for r in c.rows])
    assert np.array_equal(np.isnan(aa), nan_row[c.links[1]])
    assert np.any(nan_row[c.links[0]] & ~nan_row[c.links[1]])
    cn = R.cn(c.A_signed, c.links)
    assert (cn < 0).any() and (cn > 0).any()        # the ±1 terms cancel


def test_sink_graphs_have_sinks_orphans_and_in_rows_0_to_9():
    import heuristics_cases as K

    assert {(n + 15) // 16 for n in K.SINK_NS} >= {1, 2, 64, 65}
    assert {1, 15, 16, 17, 1024, 1025, 1041} <= set(K.SINK_NS)
    assert any((1.0 / n) * n != 1.0 for n in K.SINK_NS)
    for n in K.SINK_NS:
        g = K.sink_graph(n)
        A = g.A
        assert A.shape == (n, n) and A.has_sorted_indices and np.all(A.data > 0)
        if n == 1:
            continue
        r, indeg = np.asarray(A.sum(axis=1)).ravel(), np.diff(A.tocsc().indptr)
        assert np.array_equal(g.sinks, np.nonzero(r == 0)[0]) and np.array_equal(g.orphans, np.nonzero(indeg == 0)[0])
        assert 0.05 * n <= len(g.sinks) <= 0.2 * n or n < 20
        assert np.any(indeg[g.sinks] > 0), "a sink with in-edges: r = 0 while c > 0"
        assert len(g.orphans) >= 1 and np.any(r[g.orphans] > 0)
        assert set(range(10)) <= set(indeg.tolist())
        assert np.array_equal(indeg[g.designated], np.arange(10))
        assert 3.0 <= A.nnz / n <= 5.0
        src = K.sink_sources(g)
        assert len(src) <= 129 and np.array_equal(src, np.unique(src))
        kinds = (np.isin(src, g.sinks), np.isin(src, g.orphans), ~np.isin(src, np.r_[g.sinks, g.orphans]))
        assert all(k.any() for k in kinds) and np.any(kinds[0] & (indeg[src] > 0))
    A = K.star(70000)
    assert A.shape == (70001, 70001) and A.nnz == 140000 and (A != A.T).nnz == 0 and A[0].nnz == 70000


@pytest.mark.parametrize("n", [1, 15, 16, 17, 49, 1024, 1025, 1041])
def test_fixed_iteration_runs_stop_where_the_gpu_test_assumes(n):
    """tol = 0, max_iter = k: every source that is not a sink runs exactly k iterations, in the batched form and in
    the literal loop alike, and the two give the same iterate."""
    import heuristics_cases as K

    g = K.sink_graph(n)
    src = K.sink_sources(g)
    sink = np.isin(src, g.sinks)
    exact = (1.0 / n) * n == 1.0
    for k in K.FIXED_KS:
        X, its = R.ppr_batched(g.A, src, tol=0.0, max_iter=k)
        assert n == 1 or np.all(its[~sink] == k), (n, k, its)   # one node alone is a fixed point from the start
        if exact:
            assert np.all(its[sink] == 1)          # s·(zᵀs) reproduces s: the first step changes nothing
        ops = R._operators(g.A, 0.85)
        for j in np.r_[np.nonzero(sink)[0][:3], np.nonzero(~sink)[0][:5]]:
            x, it = R.pagerank_power(g.A, int(src[j]), tol=0.0, max_iter=k, ops=ops)
            assert it == its[j] and np.allclose(X[:, j], x, rtol=1e-12, atol=0)
    if n == 1041:
        # the freeze test: with a coarse tol the columns stop on either side of the host's check at 8
        _, its = R.ppr_batched(g.A, src, tol=K.COARSE_TOL, max_iter=100)
        assert its.min() < 8 < its.max() < 100 and len(np.unique(its)) >= 4, np.unique(its)
