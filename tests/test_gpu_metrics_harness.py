"""harness.fit_and_select on the USAir split: every epoch's reported (valid, test) pair is the numpy restatement
(tests/metrics_reference.py) of that epoch's `net.score` output, the selected epoch is the first maximum of the validation
column, and the loop leaves `train_and_evaluate_fused` where it was.  The trainer is bit-reproducible for one seed
(tests/test_gpu_signnet.py), so a second trainer stepped by hand gives the scores the loop saw."""
import numpy as np
import pytest
import torch

import metrics_reference as ref

pytestmark = pytest.mark.gpu

EPOCHS, SEED, LR, HIDDEN, M_NEG = 3, 1, 2e-3, 256, 10


@pytest.fixture(scope="module")
def usair():
    from s3grl_amd import workloads
    from s3grl_amd.engine import Engine

    w = workloads.make("usair_pos_k2")
    eng = Engine("cuda:0")
    G, f = eng.graph(w.A), eng.features(w.X)

    def rows_of(pos, neg):
        li = np.concatenate([pos, neg], axis=1)
        y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
        res = eng.precompute(G, f, eng.links(li), mode="pos", num_hops=1, sign_k=2)
        return res.rows, res.row_ptr, y

    out = {s: rows_of(*w.split.links[s]) for s in ("train", "valid", "test")}
    rng = np.random.default_rng(0)
    n = w.split.num_nodes
    for s in ("valid", "test"):              # M_NEG negatives per positive, in row order, for 'mrr'
        pos = w.split.links[s][0]
        neg = rng.integers(0, n, size=(2, pos.shape[1] * M_NEG))
        neg[1] = np.where(neg[0] == neg[1], (neg[1] + 1) % n, neg[1])
        out[s + "_mrr"] = rows_of(pos, neg)
    yield out
    eng.close()


def reference_results(eval_metric, scores, y):
    s, y = scores.cpu().numpy(), y.cpu().numpy()
    pos, neg = s[y == 1], s[y == 0]
    if eval_metric == "auc":
        return {"AUC": ref.roc_auc(y, s), "AP": ref.average_precision(y, s)}
    if eval_metric == "hits":
        return {f"Hits@{k}": ref.hits_at(pos, neg, k) for k in (20, 50, 100)}
    return {"MRR": ref.mrr(pos, neg.reshape(pos.size, -1))["MRR"]}


# abs bounds of tests/test_gpu_metrics.py: AUC 1e-12, AP 1e-11 (n·2^-53 is far below at these sizes), Hits exact (the same
# integer division), the MRR mean P·2^-53 with P < 1000
TOL = {"AUC": 1e-12, "AP": 1e-11, "Hits@20": 0.0, "Hits@50": 0.0, "Hits@100": 0.0, "MRR": 1000 * 2.0 ** -53}


@pytest.mark.parametrize("eval_metric", ["auc", "hits", "mrr"])
def test_every_epoch_is_the_reference_on_that_epochs_scores(usair, eval_metric):
    from s3grl_amd.harness import fit_and_select
    from s3grl_amd.signnet import SIGNNetTrainer

    sfx = "_mrr" if eval_metric == "mrr" else ""
    train, valid, test = usair["train"], usair["valid" + sfx], usair["test" + sfx]
    out = fit_and_select(train, valid, test, eval_metric=eval_metric, hidden=HIDDEN, epochs=EPOCHS, lr=LR, seed=SEED)
    hist = out["history"]
    assert all(len(h) == EPOCHS for h in hist.values())

    rows, row_ptr, y = train
    net = SIGNNetTrainer(rows.shape[1] * rows.shape[2], HIDDEN, 0, "", 0.5, LR, seed=SEED, device=rows.device)
    rows, row_ptr, yf = net._store(rows, row_ptr, y)
    for e in range(EPOCHS):
        net._epoch(rows, row_ptr, yf, 32)
        want = [reference_results(eval_metric, net.score(s[0], s[1]), s[2]) for s in (valid, test)]
        assert set(want[0]) == set(hist)
        for key in hist:
            print(eval_metric, e, key, hist[key][e], (want[0][key], want[1][key]))
            assert abs(hist[key][e][0] - want[0][key]) <= TOL[key]
            assert abs(hist[key][e][1] - want[1][key]) <= TOL[key]
    net.close()

    for key, h in hist.items():
        col = [v for v, _ in h]
        assert out["best_epoch"][key] == col.index(max(col))          # the first maximum
        assert out["selected"][key] == h[out["best_epoch"][key]][1]
    assert out["trainer"].epochs_done == EPOCHS
    out["trainer"].close()


def test_the_fused_harness_reports_what_it_did(usair):
    from s3grl_amd.harness import fit_and_select, train_and_evaluate_fused

    kw = dict(hidden=HIDDEN, epochs=EPOCHS, lr=LR, seed=SEED)
    auc, net = train_and_evaluate_fused(usair["train"], usair["test"], **kw)
    net.close()
    out = fit_and_select(usair["train"], usair["valid"], usair["test"], eval_metric="auc", **kw)
    out["trainer"].close()
    # the same scores; `auc_score` averages fp64 ranks, the metrics unit divides an exact integer once: 1e-12 covers both
    assert abs(out["history"]["AUC"][-1][1] - auc) <= 1e-12
    auc2, net2 = train_and_evaluate_fused(usair["train"], usair["test"], **kw)
    net2.close()
    assert auc2 == auc                                                # scoring in between changes no later result
