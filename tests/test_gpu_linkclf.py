"""The link classifier of the N2V row on the GPU (s3grl_amd/linkclf.py): the ladder from a start where the full step is
rejected, a separable input, a table of scale 0.05, rows past the block cap, sklearn's recorded predictions, a live
node2vec table read in place, and every argument check that needs a device.  Bounds and inputs: tests/linkclf_checks.py;
the float64 restatement: tests/linkclf_reference.py."""
from pathlib import Path

import numpy as np
import pytest
import torch

import linkclf_checks as K
import linkclf_reference as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"


def _theta(clf):
    return np.r_[clf.coef_[0], clf.intercept_]


def test_rejected_full_step_walks_the_ladder():
    """From 20 θ* the restatement halves t (tests/test_linkclf_host.py asserts it): five teacher-forced steps take its
    rungs, and the fit from there ends at θ* in its number of iterations."""
    from s3grl_amd import linkclf as L

    emb, pairs, y = K.make_input(**K.REJECTED)
    Z, yf = R.features(emb, pairs), y.astype(np.float64)
    star, _ = R.optimum(Z, yf)
    worst, ts = {}, []
    clf = L.LinkClassifier(emb.shape[1], max_iter=0)
    clf.fit(emb, pairs, y, init=20 * star)                  # max_iter = 0: θ is set, nothing runs
    assert np.array_equal(_theta(clf), 20 * star) and clf.n_iter_ == 0 and not clf.converged_
    for step in range(5):
        s, _ = K.step_check(clf, emb, pairs, y, worst, f"rejected step {step}")
        ts.append(s["step_t"])
    assert min(ts) < 1.0 and ts[0] < 1.0, ts
    full = L.LinkClassifier(emb.shape[1])
    K.fit_check(full, emb, pairs, y, worst, "rejected fit", init=20 * star)
    print("rejected", ts, {k: f"{v:.2g}" for k, v in worst.items()})
    clf.close()
    full.close()


@pytest.mark.parametrize("name", ["SEPARABLE", "TINY_SCALE"])
def test_separable_and_small_scale_inputs(name):
    from s3grl_amd import linkclf as L

    emb, pairs, y = K.make_input(**getattr(K, name))
    worst = {}
    clf = L.LinkClassifier(emb.shape[1])
    for step in range(3):
        K.step_check(clf, emb, pairs, y, worst, f"{name} step {step}")
    K.fit_check(clf, emb, pairs, y, worst, name)
    print(name, {k: f"{v:.2g}" for k, v in worst.items()})
    clf.close()


def test_more_tiles_than_blocks():
    """M past max_blocks · rows_per_block: every block of the two row passes takes two tiles, the last tile one row."""
    from s3grl_amd import linkclf as L

    D = 8
    M = K.many_tiles(L.layout(D))
    emb, pairs, y = K.make_input(D, M, seed=2)
    worst = {}
    clf = L.LinkClassifier(D)
    K.step_check(clf, emb, pairs, y, worst, "many tiles step")
    K.fit_check(clf, emb, pairs, y, worst, "many tiles fit")
    print("many tiles", M, {k: f"{v:.2g}" for k, v in worst.items()})
    clf.close()


@pytest.mark.parametrize("name", ["d8", "d32", "d33"])
def test_hard_predictions_are_default_sklearns(name):
    """tests/golden/linkclf_*.npz (sklearn 1.7.2 on the CPU): the engine's hard predictions are default
    LogisticRegression's on every row but those where default and run-to-convergence sklearn differ in the file itself,
    and its θ is the run-to-convergence one to lbfgs's own precision."""
    from s3grl_amd import linkclf as L

    f = np.load(GOLDEN / f"linkclf_{name}.npz")
    emb, pairs, y = f["emb"], f["pairs"], f["labels"]
    clf = L.LinkClassifier(emb.shape[1]).fit(emb, pairs, y)
    pred = clf.predict(emb, pairs).cpu().numpy()
    differ = f["default_predict"] != f["tight_predict"]
    assert differ.sum() <= 0.01 * len(y)
    assert np.array_equal(pred[~differ], f["default_predict"][~differ])
    assert np.array_equal(pred, f["tight_predict"])
    assert np.max(np.abs(_theta(clf) - np.r_[f["tight_coef"], f["tight_intercept"]])) < 2e-5
    assert clf.confusion(emb, pairs, y) == R.confusion(f["tight_predict"], y)
    clf.close()


def test_reads_a_live_node2vec_table_in_place():
    """`Node2Vec._table()` hands out the trainer's own weight: a fit through it equals a fit on `embedding()`'s copy bit
    for bit, sees the next epoch's update without a new accessor call, and changes nothing in the table."""
    from s3grl_amd import linkclf as L
    from s3grl_amd.node2vec import Node2Vec

    rng = np.random.default_rng(0)
    n, D = 40, 8
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n])
    n2v = Node2Vec(np.concatenate([ring, ring[::-1]], axis=1), n, D, seed=3)
    pairs = rng.integers(0, n, size=(90, 2))
    y = (rng.random(90) < 0.5).astype(np.uint8)
    table = n2v._table()
    assert (table.num_nodes, table.dim) == (n, D)
    thetas = []
    for epoch in range(2):
        n2v.fit(1)
        before = n2v.embedding().clone()
        live = L.LinkClassifier(D).fit(table, pairs, y)
        copy = L.LinkClassifier(D).fit(before, pairs, y)
        assert np.array_equal(_theta(live), _theta(copy))
        assert torch.equal(live.predict(table, pairs), copy.predict(before, pairs))
        assert torch.equal(n2v.embedding(), before)
        thetas.append(_theta(live))
        live.close()
        copy.close()
    assert not np.array_equal(thetas[0], thetas[1])
    with pytest.raises(ValueError, match=r"\[N, 9\]"):
        L.LinkClassifier(9).fit(table, pairs, y)
    n2v.close()


def test_argument_checks_on_the_device():
    from s3grl_amd import linkclf as L

    emb, pairs, y = K.make_input(8, 20, seed=0)
    clf = L.LinkClassifier(8)
    with pytest.raises(RuntimeError, match="not fitted"):
        clf.predict(emb, pairs)
    for labels in (np.ones(20, dtype=np.uint8), np.zeros(20, dtype=np.uint8)):
        with pytest.raises(ValueError, match="one class"):
            clf.fit(emb, pairs, labels)
        with pytest.raises(ValueError, match="one class"):
            clf.newton_step(emb, pairs, labels)
    bad = pairs.copy()
    bad[7, 1] = K.HUB_N
    with pytest.raises(ValueError, match="outside"):
        clf.fit(emb, bad, y)
    with pytest.raises(ValueError, match="one label per pair"):
        clf.fit(emb, pairs, y[:-1])
    with pytest.raises(ValueError, match=r"\[N, 8\]"):
        clf.fit(emb[:, :7], pairs, y)
    with pytest.raises(ValueError, match="init must be"):
        clf.fit(emb, pairs, y, init=np.zeros(8))
    with pytest.raises(ValueError, match="empty"):
        clf.fit(emb, pairs[:0], y[:0])
    clf.fit(emb, pairs, y)
    with pytest.raises(ValueError, match="outside"):
        clf.predict(emb, bad)
    assert clf.predict(emb, pairs[:0]).shape == (0,) and clf.confusion(emb, pairs[:0], y[:0]) == (0, 0, 0, 0)
    tp, fp, fn, tn = clf.confusion(emb, pairs, y)
    assert tp + fn == int(y.sum()) and fp + tn == int((1 - y).sum())
    # the C ABI checks on its own: a label vector of one class, a node outside the table
    from s3grl_amd import _native as N

    dev = clf.engine.device
    e = torch.as_tensor(emb).to(dev)
    p = torch.as_tensor(bad).to(device=dev, dtype=torch.int32)
    ones = torch.ones(20, dtype=torch.uint8, device=dev)
    yy = torch.as_tensor(y).to(dev)
    good = torch.as_tensor(pairs).to(device=dev, dtype=torch.int32)
    for rows, labels in ((p, yy), (good, ones)):
        with pytest.raises(ValueError):
            N.check(N.lib().s3grl_linkclf_fit(clf._h, N.ptr(e), K.HUB_N, N.ptr(rows), N.ptr(labels), 20, None), "fit")
    clf.close()
    with pytest.raises(RuntimeError, match="closed"):
        clf.predict(emb, pairs)
