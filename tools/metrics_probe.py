"""Link metrics probe -> profiles/metrics_probe.json.

Ranked path, at the headline list's 164 000 scores and the collab-scale 1 000 000 scores (half positives, seeded normal
scores and, as the tied flavour, common-neighbour-like counts): the wall time of `LinkMetrics.ranked` from a device tensor
of scores to host numbers, next to `harness.auc_score` (eager torch, AUC only) and `heuristics.evaluate_auc` (numpy, fed
the same device tensor, so with its copy) on the same machine.  MRR path, at P = 86 596 with M = 1 000 (the
ogbl-citation2 validation shape) and P = 100 000 with M = 100: the wall time of `LinkMetrics.mrr` and the bytes it has to
read (4·P·(M + 1)) over that time, as a fraction of the 8.0 TB/s HBM figure.  Every time is a host clock around a call
that ends with its results on the host, the median of --repeats calls after --warmup calls.

    python tools/metrics_probe.py [--out profiles/metrics_probe.json] [--repeats 20] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from s3grl_amd import harness, heuristics, metrics  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def median_s(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def ranked_probe(lm, n, flavour, warmup, repeats):
    g = torch.Generator(device="cuda").manual_seed(n)
    y = (torch.arange(n, device="cuda") % 2 == 0).to(torch.int64)
    if flavour == "normal":
        s = torch.randn(n, device="cuda", generator=g) + 0.5 * y
    else:                                       # mostly zero counts, as common neighbours are
        s = torch.where(torch.rand(n, device="cuda", generator=g) < 0.85, 0.0,
                        torch.poisson(torch.full((n,), 2.0, device="cuda"), generator=g)) + 2.0 * y
    yf = y.to(torch.float32)
    r = lm.ranked(s, y, ks=(20, 50, 100))
    old = harness.auc_score(s, y)
    ref = heuristics.evaluate_auc(s, yf, s, yf)
    out = {"n": n, "thresholds": r["thresholds"], "AUC": r["AUC"], "AP": r["AP"],
           "auc_minus_harness_auc_score": r["AUC"] - old, "auc_minus_numpy": r["AUC"] - ref["AUC"][0],
           "ap_minus_numpy": r["AP"] - ref["AP"][0],
           "ranked_auc_ap_hits_s": median_s(lambda: lm.ranked(s, y, ks=(20, 50, 100)), warmup, repeats),
           "harness_auc_score_s": median_s(lambda: harness.auc_score(s, y), warmup, repeats),
           "numpy_auc_ap_one_split_s": median_s(lambda: (heuristics.roc_auc(yf, s), heuristics.average_precision(yf, s)),
                                                warmup, max(3, repeats // 4))}
    out["speedup_vs_harness_auc_score"] = out["harness_auc_score_s"] / out["ranked_auc_ap_hits_s"]
    out["speedup_vs_numpy"] = out["numpy_auc_ap_one_split_s"] / out["ranked_auc_ap_hits_s"]
    return out


def mrr_probe(lm, P, M, warmup, repeats):
    g = torch.Generator(device="cuda").manual_seed(P + M)
    pos = torch.randn(P, device="cuda", generator=g) + 1.0
    neg = torch.randn(P, M, device="cuda", generator=g)
    r = lm.mrr(pos, neg)
    t = median_s(lambda: lm.mrr(pos, neg), warmup, repeats)
    nbytes = 4 * P * (M + 1)
    return {"P": P, "M": M, "rows_per_wave": metrics.layout(M)["rows_per_wave"], "MRR": r["MRR"], "hits@10": r["hits@10"],
            "mrr_s": t, "bytes_read": nbytes, "bytes_per_s": nbytes / t, "fraction_of_8_TB_per_s": nbytes / t / HBM_BYTES_PER_S}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "metrics_probe.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lm = metrics.LinkMetrics("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup,
           "layout": metrics.layout(), "ranked": {}, "mrr": []}
    for n in (164_000, 1_000_000):
        for flavour in ("normal", "counts"):
            r = ranked_probe(lm, n, flavour, args.warmup, args.repeats)
            res["ranked"][f"{n}_{flavour}"] = r
            print("ranked", n, flavour, json.dumps(r), flush=True)
    for P, M in ((86_596, 1000), (100_000, 100)):
        r = mrr_probe(lm, P, M, args.warmup, args.repeats)
        res["mrr"].append(r)
        print("mrr", json.dumps(r), flush=True)
    lm.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
