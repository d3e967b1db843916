"""Side-by-side SIGNNet runs probe: seconds per group epoch of `SIGNNetRuns` (R runs in four launches
per step) against R sequential lone `SIGNNetTrainer` epochs, for R in 1, 2, 4, 8, 10, on the train split of USAir PoS
sign_k=2 and of PubMed PoS sign_k=3; hidden 256, batches of 32, dropout 0.5.  Both paths are timed in the same process,
alternating, three repeats each, after a warm-up epoch of each configuration; host clock from the first call to the
read-back of the losses; the profiler is off.  The margin of a comparison is the spread (max - min) of the three repeats
of the lone path.  The members and the lone trainers have the same seeds, so their losses are compared bit for bit on
the way.

    python tools/signnet_runs_probe.py [--out profiles/signnet_runs_probe.json] [--runs 1 2 4 8 10] [--repeats 3]
    python tools/signnet_runs_probe.py --only-group pubmed_pos_k3 --runs 4 --epochs 3

`--only-group NAME` runs nothing but group epochs of one workload at one R: the run to put under `rocprofv3
--kernel-trace --stats` (no counters) for the per-kernel times.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))

from signnet_probe import CFG, WORKLOADS, train_split      # noqa: E402  (the lone probe's config and splits)

RUNS = (1, 2, 4, 8, 10)


def make(train, seeds, group):
    from s3grl_amd.signnet import SIGNNetRuns, SIGNNetTrainer

    in_width = train[0].shape[1] * train[0].shape[2]
    if group:
        return SIGNNetRuns(in_width, CFG["hidden"], dropout=CFG["dropout"], lr=CFG["lr"], seeds=seeds)
    return [SIGNNetTrainer(in_width, CFG["hidden"], dropout=CFG["dropout"], lr=CFG["lr"], seed=s) for s in seeds]


def group_epoch(group, store):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = group._epoch(*store, CFG["batch_size"]).cpu()
    return time.perf_counter() - t0, losses


def lone_epochs(lones, store):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = torch.stack([net._epoch(*store, CFG["batch_size"]) for net in lones]).cpu()
    return time.perf_counter() - t0, losses


def compare(train, R, repeats):
    seeds = list(range(1, R + 1))
    group, lones = make(train, seeds, True), make(train, seeds, False)
    store = group.members[0]._store(*train)
    same = torch.equal(group_epoch(group, store)[1], lone_epochs(lones, store)[1])      # the warm-up epoch of each
    g, lone = [], []
    for _ in range(repeats):
        tg, lg = group_epoch(group, store)
        tl, ll = lone_epochs(lones, store)
        same = same and torch.equal(lg, ll)
        g.append(tg)
        lone.append(tl)
    group.close()
    for net in lones:
        net.close()
    gm, lm = sorted(g)[len(g) // 2], sorted(lone)[len(lone) // 2]
    margin = max(lone) - min(lone)
    verdict = "group faster" if lm - gm > margin else ("lone faster" if gm - lm > margin else "no difference")
    return {"runs": R, "group_s": g, "lone_s": lone, "group_s_median": gm, "lone_s_median": lm, "lone_spread_s": margin,
            "lone_over_group": lm / gm, "verdict": verdict, "losses_bit_identical": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "signnet_runs_probe.json"))
    ap.add_argument("--runs", type=int, nargs="+", default=list(RUNS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--only-group", default="")
    a = ap.parse_args()
    if a.only_group:
        train, _, eng = train_split(a.only_group)
        group = make(train, list(range(1, a.runs[0] + 1)), True)
        store = group.members[0]._store(*train)
        spent = [group_epoch(group, store)[0] for _ in range(a.epochs)]
        print(json.dumps({"workload": a.only_group, "runs": a.runs[0], "group_epoch_s": spent}))
        group.close()
        eng.close()
        return
    res = {"config": CFG, "repeats": a.repeats, "clock": "host, first call to the read-back of the losses",
           "margin": "max - min of the lone path's repeats", "workloads": {}}
    for name in WORKLOADS:
        train, _, eng = train_split(name)
        L = train[2].numel()
        res["workloads"][name] = {"links": L, "steps_per_epoch": -(-(L - 1) // CFG["batch_size"]),
                                  "in_width": int(train[0].shape[1] * train[0].shape[2]),
                                  "by_runs": [compare(train, R, a.repeats) for R in a.runs]}
        print(name, json.dumps(res["workloads"][name]), flush=True)
        del train
        eng.close()
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
