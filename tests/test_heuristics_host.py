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
