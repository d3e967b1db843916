"""N2V row probe:
  * the 50-epoch row on the USAir split (hidden 32, one negative, batches of 32, lr 0.01, a fresh classifier every
    epoch): the (val, test) AUC and AP of every epoch, the Logger's choice after 3 and after 50 epochs, the host clock
    around the row, and the Newton iterations every fit took
  * at PubMed size (the packaged topology, its train links and as many negatives, D = 32, the table one node2vec
    epoch leaves): the host clock around one fit plus the two predict-and-count calls of an evaluation, each ending in
    a device read-back, median of five after a warm-up, next to the clock around one node2vec epoch on the same graph

    python tools/n2v_row_probe.py [--out profiles/n2v_row_probe.json] [--only-row | --only-pubmed]

`--only-row` runs nothing but the USAir row, `--only-pubmed` nothing but the PubMed-size part: the runs to put under
`rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

CFG = dict(hidden=32, neg_ratio=1, batch_size=32, lr=0.01, epochs=50, seed=1)


def usair_row(epochs):
    from s3grl_amd import n2v, workloads as W
    from s3grl_amd.gae import best_at_first_max

    n, e = W.load_topology("usair")
    split = W.edge_split(n, e, seed=1)
    se = split.split_edge()
    iters = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    results = n2v._train_run(np.asarray(se["train"]["edge"]).T, n, se, epochs=epochs, hidden=CFG["hidden"],
                             neg_ratio=CFG["neg_ratio"], batch_size=CFG["batch_size"], lr=CFG["lr"], eval_steps=1,
                             seed=CFG["seed"], device=None,
                             on_eval=lambda ep, loss, res, t, clf, lists: iters.append(clf.n_iter_))
    spent = time.perf_counter() - t0
    pick = lambda k, upto: [float(v) for v in best_at_first_max(results[k][:upto])]   # noqa: E731
    return {"train_rows": int(len(se["train"]["edge"]) + len(se["train"]["edge_neg"])), "row_s": spent,
            "newton_iterations": iters, "AUC_per_epoch": results["AUC"], "AP_per_epoch": results["AP"],
            "after_3_epochs": {k: pick(k, 3) for k in results},
            f"after_{epochs}_epochs": {k: pick(k, epochs) for k in results}}


def pubmed_fit():
    from s3grl_amd import workloads as W
    from s3grl_amd.linkclf import LinkClassifier
    from s3grl_amd.n2v import _labelled
    from s3grl_amd.node2vec import Node2Vec

    n, e = W.load_topology("pubmed")
    split = W.edge_split(n, e, seed=1)
    se = split.split_edge()
    n2v = Node2Vec(np.asarray(se["train"]["edge"]).T, n, CFG["hidden"], seed=CFG["seed"])
    dev = n2v.engine.device
    lists = {s: tuple(t.to(dev) for t in _labelled(se, s, n)) for s in ("train", "valid", "test")}
    n2v.fit(1)                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n2v.fit(1)                                                   # ends in a read-back of the losses
    epoch_s = time.perf_counter() - t0
    table = n2v._table()
    times, iters = [], None
    for rep in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf = LinkClassifier(CFG["hidden"]).fit(table, *lists["train"])
        t1 = time.perf_counter()
        counts = [clf.confusion(table, *lists[s]) for s in ("valid", "test")]
        t2 = time.perf_counter()
        iters = clf.n_iter_
        clf.close()
        if rep:
            times.append((t1 - t0, t2 - t1))
    n2v.close()
    fit_s, pred_s = (float(np.median([t[i] for t in times])) for i in (0, 1))
    return {"num_nodes": n, "train_rows": int(lists["train"][0].shape[0]),
            "valid_rows": int(lists["valid"][0].shape[0]), "test_rows": int(lists["test"][0].shape[0]),
            "newton_iterations": iters, "fit_s": fit_s, "two_predicts_s": pred_s, "node2vec_epoch_s": epoch_s,
            "share_of_an_epoch": (fit_s + pred_s) / (fit_s + pred_s + epoch_s), "counts": counts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "n2v_row_probe.json"))
    ap.add_argument("--only-row", action="store_true")
    ap.add_argument("--only-pubmed", action="store_true")
    a = ap.parse_args()
    if a.only_row:
        print(json.dumps({"row_s": usair_row(CFG["epochs"])["row_s"]}))
        return
    if a.only_pubmed:
        print(json.dumps(pubmed_fit()))
        return
    usair_row(1)                                                 # warm-up
    res = {"config": CFG, "usair": usair_row(CFG["epochs"]), "pubmed": pubmed_fit()}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res)[:4000])


if __name__ == "__main__":
    main()
