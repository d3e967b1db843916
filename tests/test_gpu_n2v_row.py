"""The N2V row end to end (s3grl_amd/n2v.py) on the packaged USAir topology, 3 epochs: at every epoch the logged AUC /
AP are what the float64 restatement of the classifier (tests/linkclf_reference.py), refitted on the trainer's own
embedding, gives through the curve-based metrics; two runs with one seed agree; `run_n2v` returns and logs what the
reference's loop does.  No learning level is asserted here: DESIGN §17 records the measured one."""
from types import SimpleNamespace

import numpy as np
import pytest

import linkclf_checks as K
import linkclf_reference as R

pytestmark = pytest.mark.gpu
EPOCHS = 3


@pytest.fixture(scope="module")
def usair():
    from s3grl_amd import workloads

    n, e = workloads.load_topology("usair")
    return workloads.edge_split(n, e, seed=1)


def _labelled(split_edge, name):
    pos, neg = np.asarray(split_edge[name]["edge"]), np.asarray(split_edge[name]["edge_neg"])
    return np.concatenate([pos, neg]), np.r_[np.ones(len(pos), dtype=np.uint8), np.zeros(len(neg), dtype=np.uint8)]


def test_logged_metrics_are_the_restatements(usair):
    from s3grl_amd import n2v
    from s3grl_amd.gae import best_at_first_max
    from s3grl_amd.heuristics import average_precision, roc_auc

    split_edge = usair.split_edge()
    edge_index = np.asarray(split_edge["train"]["edge"]).T
    seen = []

    def on_eval(epoch, loss, res, trainer, clf, lists):
        assert np.isfinite(loss) and clf.converged_
        seen.append((epoch, res, trainer.embedding().cpu().numpy(), np.r_[clf.coef_[0], clf.intercept_],
                     {s: clf.confusion(trainer._table(), *lists[s]) for s in ("valid", "test")}))

    results = n2v._train_run(edge_index, usair.num_nodes, split_edge, epochs=EPOCHS, hidden=32, neg_ratio=1,
                             batch_size=32, lr=0.01, eval_steps=1, seed=1, device=None, on_eval=on_eval)
    assert [s[0] for s in seen] == list(range(EPOCHS)) and len(results["AUC"]) == EPOCHS
    train_pairs, train_y = _labelled(split_edge, "train")
    worst, unsure_rows = 0.0, 0
    for i, (epoch, res, emb, theta, counts) in enumerate(seen):
        assert emb.shape == (usair.num_nodes, 32) and (i == 0 or not np.array_equal(emb, seen[i - 1][2]))
        Z, yf = R.features(emb, train_pairs), train_y.astype(np.float64)
        star, gstar = R.optimum(Z, yf)
        assert gstar < 1e-10
        tb = K.fit_bound(Z, yf, star, gstar, 1.0, 1e-8)
        worst = max(worst, float(np.max(np.abs(theta - star)) / tb))
        assert np.max(np.abs(theta - star)) <= tb, f"epoch {epoch}"
        exact = True
        for s in ("valid", "test"):
            pairs, y = _labelled(split_edge, s)
            Zs = R.features(emb, pairs)
            z = R.decision(Zs, star)
            unsure = np.abs(z) <= K.z_bound(Zs, star, tb)
            unsure_rows += int(unsure.sum())
            ref = R.confusion(z > 0, y)
            slack = (int((unsure & (y == 1)).sum()), int((unsure & (y == 0)).sum()))
            tp, fp, fn, tn = counts[s]
            assert tp + fn == ref[0] + ref[2] and fp + tn == ref[1] + ref[3]
            assert abs(tp - ref[0]) <= slack[0] and abs(fp - ref[1]) <= slack[1], f"epoch {epoch} {s}"
            if unsure.any():
                exact = False
                continue
            k = 0 if s == "valid" else 1
            assert res["AUC"][k] == pytest.approx(roc_auc(y, (z > 0).astype(np.uint8)), abs=1e-13)
            assert res["AP"][k] == pytest.approx(average_precision(y, (z > 0).astype(np.uint8)), abs=1e-13)
        assert results["AUC"][i] == res["AUC"] and results["AP"][i] == res["AP"]
        assert exact or unsure_rows
    print("n2v row: worst |θ − θ*| / bound", f"{worst:.2g}", "rows inside the z bound", unsure_rows,
          "AUC (val, test) per epoch", [tuple(round(v, 4) for v in r) for r in results["AUC"]])
    # two more runs through the public entry: identical, and the Logger's choice over the three epochs above
    a = n2v.run_n2v_row(usair, epochs=EPOCHS, seed=1)
    b = n2v.run_n2v_row(usair, epochs=EPOCHS, seed=1)
    assert a == b and set(a) == {"AUC", "AP"}
    for key in a:
        assert a[key] == tuple(float(v) for v in best_at_first_max(results[key]))
        assert 0.0 <= a[key][1] <= 1.0


def test_run_n2v_returns_and_logs_as_the_reference(usair, tmp_path, capsys):
    from s3grl_amd import n2v

    split_edge = usair.split_edge()
    data = SimpleNamespace(num_nodes=usair.num_nodes, edge_index=np.asarray(split_edge["train"]["edge"]).T)
    args = SimpleNamespace(res_dir=str(tmp_path), runs=1, eval_steps=1, log_steps=1, epochs=2)
    auc = n2v.run_n2v(None, data, split_edge, 2, 0.01, 32, 1, 32, 4, args, 1)
    row = n2v.run_n2v_row(usair, epochs=2, seed=1)
    assert auc == pytest.approx(100 * row["AUC"][1], abs=1e-4)           # fp32 · 100, as the Logger holds it
    out = capsys.readouterr()
    assert out.out == "" and out.err == ""
    lines = (tmp_path / "log.txt").read_text().splitlines()
    assert lines[0] == "AUC" and lines[2] == "AP" and len(lines) == 8
    assert lines[1].startswith("Run: 01, Epoch: 00, Loss: ") and lines[5].startswith("Run: 01, Epoch: 01, Loss: ")
    assert "Valid: " in lines[1] and lines[1].endswith("%")
    quiet = SimpleNamespace(res_dir="", runs=1, eval_steps=2, log_steps=1)
    assert isinstance(n2v.run_n2v(None, data, split_edge, 1, 0.01, 32, 1, 32, 0, quiet, 1), float)
