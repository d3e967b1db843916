"""Host checks of the N2V row's link classifier (no GPU): the float64 restatement (tests/linkclf_reference.py) reaches
the optimum on every input of the GPU shape list and its decisions there are clear of rounding; it agrees with sklearn
run to convergence; the lane layouts and tile edges the shape list reaches; how far outside the GPU tests' bounds each
plausible kernel fault lands; `hard_auc_ap` against the curve-based metrics; every argument check; the ABI."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import linkclf_checks as K
import linkclf_reference as R

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden"
FIXTURES = ("d8", "d32", "d33")


@pytest.fixture(scope="module")
def linkclf():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd import linkclf as module

    return module


def _z(emb, pairs, y):
    return R.features(emb, pairs), np.asarray(y, dtype=np.float64)


# ---- the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", K.DIMS)
def test_restatement_reaches_the_optimum_on_the_shape_list(linkclf, D):
    """Every (D, M) of the GPU test: max|∇f| < 1e-10 at θ*, the fit from 0 converges, no convergence test and no rung
    choice on the way lies within the engine's rounding of the other outcome, and no row's z lies within the bound on
    z (so predictions and counts can be compared exactly)."""
    for M in K.row_counts(linkclf.layout(D)["rows_per_block"]):
        emb, pairs, y = K.make_input(D, M, seed=1)
        assert set(np.unique(y)) == {0, 1}
        Z, yf = _z(emb, pairs, y)
        star, gstar = R.optimum(Z, yf)
        assert gstar < 1e-10, (D, M, gstar)
        fit, clear = K.unambiguous(Z, yf, 1.0, 1e-8)
        assert clear and fit["done"] == R.CONVERGED and 2 <= fit["n_iter"] <= 12, (D, M, fit["n_iter"])
        tb = K.fit_bound(Z, yf, star, gstar, 1.0, 1e-8)
        assert np.max(np.abs(fit["theta"] - star)) <= tb
        assert (np.abs(R.decision(Z, star)) > K.z_bound(Z, star, tb)).all(), (D, M)


def test_inputs_hold_what_they_promise():
    emb, pairs, y = K.make_input(32, 65, seed=1)
    assert tuple(pairs[3]) == (5, 5) and tuple(pairs[6]) == tuple(pairs[7]) and (y[6], y[7]) == (1, 0)
    assert (np.any(pairs == 0, axis=1)).mean() >= 0.7 and not np.any(pairs == K.HUB_N - 1)
    assert 0.3 < y.mean() < 0.8
    # the separable input: with the ridge all but gone (C = 1e6) every row is on its own side and θ is 20 times longer
    emb, pairs, y = K.make_input(**K.SEPARABLE)
    Z, yf = _z(emb, pairs, y)
    star, gstar = R.optimum(Z, yf)
    loose = R.fit(Z, yf, C=1e6, tol=1e-6, max_iter=100)
    assert gstar < 1e-10 and np.array_equal(R.predict(Z, loose["theta"]), y)
    assert np.linalg.norm(loose["theta"]) > 20 * np.linalg.norm(star)
    assert K.unambiguous(Z, yf, 1.0, 1e-8)[1]
    # the small-scale input: H is the ridge but for the intercept's row and column
    emb, pairs, y = K.make_input(**K.TINY_SCALE)
    Z, yf = _z(emb, pairs, y)
    H = R.grad_hess(Z, yf, np.zeros(Z.shape[1]))[1]
    assert np.max(np.abs(H[:-1, :-1] - np.eye(Z.shape[1] - 1))) < 1e-3
    assert K.unambiguous(Z, yf, 1.0, 1e-8)[1]


def test_full_step_is_rejected_from_twenty_theta_star():
    """From θ = 0 the full Newton step is accepted throughout (the shape-list test above sees t = 1 only), so the ladder
    needs a start of its own: from 20 θ* the restatement halves t at least once, and clear of rounding."""
    emb, pairs, y = K.make_input(**K.REJECTED)
    Z, yf = _z(emb, pairs, y)
    assert all(s["t"] == 1.0 for s in R.fit(Z, yf)["steps"] if s["k"] is not None)
    star, _ = R.optimum(Z, yf)
    fit, clear = K.unambiguous(Z, yf, 1.0, 1e-8, init=20 * star)
    ts = [s["t"] for s in fit["steps"] if s["k"] is not None]
    assert clear and fit["done"] == R.CONVERGED and min(ts) < 1.0 and ts[0] < 1.0, ts
    assert np.max(np.abs(fit["theta"] - star)) <= K.fit_bound(Z, yf, star, 0.0, 1.0, 1e-8)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_are_what_the_generator_makes(name):
    f = np.load(GOLDEN / f"linkclf_{name}.npz")
    D, M = f["emb"].shape[1], len(f["pairs"])
    assert D in (8, 32, 33) and M <= 600 and f["emb"].dtype == np.float32 and f["labels"].dtype == np.uint8
    differ = f["default_predict"] != f["tight_predict"]
    assert differ.sum() <= 0.01 * M
    # the restatement's hard predictions are the tight fit's, and default sklearn's but for the rows left out
    Z, yf = _z(f["emb"], f["pairs"], f["labels"])
    star, gstar = R.optimum(Z, yf)
    assert gstar < 1e-10
    pred = R.predict(Z, star)
    assert np.array_equal(pred, f["tight_predict"])
    assert np.array_equal(pred[~differ], f["default_predict"][~differ])
    # default lbfgs stops a few 1e-3 away; run to convergence it lands on the restatement's θ*
    default = np.r_[f["default_coef"], f["default_intercept"]]
    tight = np.r_[f["tight_coef"], f["tight_intercept"]]
    assert 1e-5 < np.max(np.abs(default - star)) < 5e-2
    assert np.max(np.abs(tight - star)) < 2e-5


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_agrees_with_sklearn_run_to_convergence(name):
    pytest.importorskip("sklearn")
    from sklearn.linear_model import LogisticRegression

    f = np.load(GOLDEN / f"linkclf_{name}.npz")
    Z, yf = _z(f["emb"], f["pairs"], f["labels"])
    clf = LogisticRegression(tol=1e-12, max_iter=100000).fit(Z[:, :-1], f["labels"])
    star, _ = R.optimum(Z, yf)
    # lbfgs at tol = 1e-12 stops where its line search stalls: 1e-8 .. 5e-6 from θ* on inputs like these
    assert np.max(np.abs(np.r_[clf.coef_[0], clf.intercept_] - star)) < 2e-5
    assert np.array_equal(clf.predict(Z[:, :-1]), R.predict(Z, star))


# ---- layouts -------------------------------------------------------------------------------------------------------
def test_shape_list_reaches_every_layout_and_tile_edge(linkclf):
    every = {(lay["channels_per_lane"], lay["lanes_per_row"]) for lay in map(linkclf.layout, range(1, 129))}
    seen = {(lay["channels_per_lane"], lay["lanes_per_row"]) for lay in map(linkclf.layout, K.DIMS)}
    assert every == K.LAYOUTS == seen
    assert {1, 8, 31, 32, 33, 63, 64, 65, 128} <= set(K.DIMS)
    for D in K.DIMS:
        lay = linkclf.layout(D)
        assert lay["channels_per_lane"] * lay["lanes_per_row"] >= D and 256 % lay["lanes_per_row"] == 0
        r = lay["rows_per_block"]
        Ms = K.row_counts(r)
        assert {2, 63, 64, 65, r - 1, r, r + 1, 3 * r + 1} == set(Ms)
        assert min(Ms) < r and any(M % r == 0 for M in Ms) and any(M % r == 1 and M > r for M in Ms)
        assert -(-max(Ms) // r) == 4                       # more than one block, the last one a single row
        assert K.many_tiles(lay) > lay["max_blocks"] * r   # a block with two tiles, and a one-row tail
        assert K.many_tiles(lay) % r == 1
    # D + 1 against the wave (64) and against the 256 threads that share the triangle's entries
    assert {63, 64, 65} <= {D + 1 for D in K.DIMS} | set(K.DIMS)
    assert (128 + 1) * (128 + 2) // 2 > 256 > (8 + 1) * (8 + 2) // 2


# ---- faults --------------------------------------------------------------------------------------------------------
def test_every_fault_lands_far_outside_the_bounds(linkclf):
    """Each fault's worst |faulty − restatement| / bound over g, f and θ of one step from θ = 0 and of one from a
    mid-fit θ, over four listed shapes.  Measured factors at the best shape: last_block_partial_dropped 3.3e13,
    tail_rows_dropped 3.7e12, intercept_penalised 2.1e12, label_flipped 1.5e13, last_column_dropped 3.0e13,
    rung_off_by_one 1.5e13, self_pair_as_zero 2.3e13."""
    best = {f: 0.0 for f in K.FAULTS}
    for D, M in ((8, 65), (32, 128), (33, 193), (3, 64)):
        r = linkclf.layout(D)["rows_per_block"]
        emb, pairs, y = K.make_input(D, M, seed=1)
        Z, yf = _z(emb, pairs, y)
        mid = R.fit(Z, yf, max_iter=2)["theta"]
        for theta in (np.zeros(D + 1), mid):
            for fault in K.FAULTS:
                best[fault] = max(best[fault], K.fault_factor(emb, pairs, y, theta, fault, r))
    print({k: f"{v:.1e}" for k, v in best.items()})
    assert all(v >= 10 for v in best.values()), best
    emb, pairs, y = K.make_input(8, 65, seed=1)
    Z, yf = _z(emb, pairs, y)
    ref = R.newton_step(Z, yf, np.zeros(9))
    assert K.allowed_rungs(ref["margins"], K.step_bounds(Z, yf, ref, 1.0)["margins"]) == [ref["k"]]


# ---- metrics -------------------------------------------------------------------------------------------------------
def test_hard_auc_ap_is_the_curve_metrics_on_the_prediction_vector(linkclf):
    from s3grl_amd.heuristics import average_precision, roc_auc

    rng = np.random.default_rng(2)
    cases = [(rng.integers(0, 2, n), rng.integers(0, 2, n)) for n in (2, 3, 7, 40, 333) for _ in range(6)]
    y = np.array([1, 0, 1, 1, 0, 0, 1])
    cases += [(y, np.ones(7, dtype=int)), (y, np.zeros(7, dtype=int)), (y, y), (y, 1 - y)]
    checked = 0
    for y, pred in cases:
        if y.min() == y.max():
            continue
        auc, ap = linkclf.hard_auc_ap(*R.confusion(pred, y))
        assert auc == pytest.approx(roc_auc(y, pred), abs=1e-14), (y, pred)
        assert ap == pytest.approx(average_precision(y, pred), abs=1e-14), (y, pred)
        checked += 1
    assert checked > 25
    assert linkclf.hard_auc_ap(4, 0, 0, 3) == (1.0, 1.0) and linkclf.hard_auc_ap(0, 3, 4, 0)[0] == 0.0
    assert linkclf.hard_auc_ap(4, 3, 0, 0) == (0.5, 4 / 7) and linkclf.hard_auc_ap(0, 0, 4, 3) == (0.5, 4 / 7)
    for counts in ((0, 2, 0, 3), (2, 0, 3, 0)):            # one class in y_true: both curve functions refuse
        with pytest.raises(ValueError):
            linkclf.hard_auc_ap(*counts)
    with pytest.raises(ValueError):
        roc_auc(np.ones(3), np.array([1, 0, 1]))


# ---- arguments -----------------------------------------------------------------------------------------------------
def test_argument_checks(linkclf):
    T = linkclf.LinkClassifier
    for dim in (0, 129, -1):
        with pytest.raises(ValueError, match="dim must be"):
            T(dim)
        with pytest.raises(ValueError, match="dim must be"):
            linkclf.layout(dim)
    with pytest.raises(NotImplementedError, match="fit_intercept"):
        T(8, fit_intercept=False)
    for bad in (dict(C=0.0), dict(C=float("inf")), dict(tol=-1.0), dict(tol=float("nan")), dict(max_iter=-1)):
        with pytest.raises(ValueError):
            T(8, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T(8, device="cpu")


def test_run_n2v_argument_checks(linkclf):
    from s3grl_amd import n2v

    split = {s: {"edge": np.array([[0, 1], [1, 2]]), "edge_neg": np.array([[0, 2], [3, 4]])}
             for s in ("train", "valid", "test")}
    data = SimpleNamespace(num_nodes=5, edge_index=np.array([[0, 1], [1, 2]]))
    args = SimpleNamespace(res_dir="", runs=1, eval_steps=1, log_steps=1)
    call = dict(device=None, data=data, split_edge=split, epochs=0, lr=0.01, hidden_channels=8, neg_ratio=1,
                batch_size=32, num_threads=0, args=args, seed=1)
    with pytest.raises(ValueError, match="no evaluation ran"):
        n2v.run_n2v(**call)
    with pytest.raises(ValueError):
        n2v.run_n2v(**{**call, "epochs": 2, "args": SimpleNamespace(res_dir="", runs=0)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        n2v.run_n2v(**{**call, "epochs": 2, "device": "cpu"})
    with pytest.raises(ValueError, match="epochs"):
        n2v.run_n2v_row(SimpleNamespace(), epochs=0)
    for bad in (dict(hidden=200), dict(epochs=-1), dict(eval_steps=0), dict(split_edge={"train": split["train"]})):
        kw = dict(split_edge=split, epochs=1, hidden=8, neg_ratio=1, batch_size=32, lr=0.01, eval_steps=1, seed=1,
                  device=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            n2v._train_run(data.edge_index, 5, **kw)
    with pytest.raises(ValueError, match="outside"):
        n2v._train_run(data.edge_index, 4, split_edge=split, epochs=1, hidden=8, neg_ratio=1, batch_size=32, lr=0.01,
                       eval_steps=1, seed=1, device=None)


# ---- must fail without the feature ---------------------------------------------------------------------------------
def test_linkclf_is_part_of_the_abi(linkclf):
    from s3grl_amd import _native

    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_linkclf_[a-z_]+)\s*\(", header))
    assert declared == {"s3grl_linkclf_layout", "s3grl_linkclf_create", "s3grl_linkclf_fit",
                        "s3grl_linkclf_newton_step", "s3grl_linkclf_state", "s3grl_linkclf_predict",
                        "s3grl_linkclf_destroy"}
    assert declared | {"s3grl_skipgram_weight"} <= set(_native.SYMBOLS)
    assert re.search(r"\bs3grl_skipgram_weight\s*\(", header)
    for name in declared | {"s3grl_skipgram_weight"}:
        assert getattr(_native.lib(), name) is not None
    import s3grl_amd

    assert callable(s3grl_amd.run_n2v) and callable(s3grl_amd.run_n2v_row) and callable(s3grl_amd.LinkClassifier)
    assert "s3grl_linkclf.hip" in __import__("__graft_entry__").SOURCES
    src = (REPO / "s3grl_amd" / "csrc" / "s3grl_linkclf.hip").read_text()
    assert "atomicAdd(&cnt" in src and not re.search(r"atomicAdd\([^)]*(float|double)", src)
    assert "cooperative" not in src.lower() and "while (atomic" not in src
