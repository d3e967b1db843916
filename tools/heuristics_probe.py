"""Link heuristics probe -> profiles/heuristics_probe.json.

For USAir, Router (tests/golden/router_edges.txt), Cora and PubMed, each on its seed-0 train split:
  * val and test AUC / AP of CN, AA and PPR (the reference's `--use_heuristic` rows, s3grl_amd.heuristics);
  * GPU wall time of each heuristic over the four full val/test lists (host clock around the call, ending in the
    scores' read-back; a warm-up call first), PPR over every distinct source of the four lists at once;
  * PPR at block widths 64 .. 1024 next to the default width, with the iteration statistics;
  * the CPU restatement (tests/heuristics_reference.py: CN / AA in scipy on the full lists, PPR in its batched
    fp64 form) on this process's threads; PPR on --cpu-sources sampled sources, scaled by distinct / sampled.

    python tools/heuristics_probe.py [--out profiles/heuristics_probe.json] [--cpu-sources 64] [--datasets ...]
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
sys.path.insert(0, str(REPO / "tests"))

import heuristics_reference as R  # noqa: E402
from s3grl_amd import heuristics as H  # noqa: E402
from s3grl_amd import workloads as W  # noqa: E402


def split_of(name):
    if name == "router":
        n, e = W.read_seal_edges(REPO / "tests" / "golden" / "router_edges.txt")
        e = W.undirected_unique(e)
    else:
        n, e = W.load_topology(name)
    return W.edge_split(n, e, seed=0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if isinstance(out, tuple):
        out = tuple(o.cpu() for o in out)
    else:
        out = out.cpu()
    return out, time.perf_counter() - t0


def metrics(scores, lens):
    parts = np.split(np.asarray(scores, dtype=np.float64), np.cumsum(lens)[:-1])
    vt = np.r_[np.ones(lens[0]), np.zeros(lens[1])]
    tt = np.r_[np.ones(lens[2]), np.zeros(lens[3])]
    r = H.evaluate_auc(np.r_[parts[0], parts[1]], vt, np.r_[parts[2], parts[3]], tt)
    return {k: [round(v[0], 6), round(v[1], 6)] for k, v in r.items()}


def probe(name, cpu_sources, widths):
    sp = split_of(name)
    lists = [sp.links["valid"][0], sp.links["valid"][1], sp.links["test"][0], sp.links["test"][1]]
    lens = [x.shape[1] for x in lists]
    links = np.concatenate(lists, axis=1)
    src = np.unique(links[0])
    out = {"num_nodes": sp.num_nodes, "nnz": int(sp.A.nnz), "links": int(links.shape[1]),
           "distinct_sources": int(len(src))}
    h = H.Heuristics(sp.A)
    for kind, fn in (("CN", h.cn), ("AA", h.aa)):
        fn(links)
        sc, t = timed(lambda: fn(links))
        t_cpu = time.perf_counter()
        ref = (R.cn if kind == "CN" else R.aa)(sp.A, links)
        t_cpu = time.perf_counter() - t_cpu
        out[kind] = {"gpu_s": round(t, 6), "cpu_restatement_s": round(t_cpu, 4), **metrics(sc.numpy(), lens),
                     "max_abs_diff_vs_restatement": float(np.max(np.abs(sc.numpy() - ref)))}
    h.ppr(links)
    (sc, its), t = timed(lambda: h.ppr(links, return_iterations=True))
    its_src = its.numpy()[np.unique(links[0], return_index=True)[1]]
    ppr = {"gpu_s": round(t, 6), **metrics(sc.numpy(), lens),
           "iterations": {"median": float(np.median(its_src)), "mean": round(float(its_src.mean()), 2),
                          "min": int(its_src.min()), "max": int(its_src.max()),
                          "at_max_iter": int((its_src == 100).sum())}, "widths": {}}
    for bw in widths:
        (sw, _), tw = timed(lambda: h.ppr(links, block_width=bw, return_iterations=True))
        ppr["widths"][str(bw)] = {"gpu_s": round(tw, 6), "bit_equal_to_default": bool(torch.equal(sw, sc))}
    h.close()
    rng = np.random.default_rng(0)
    sample = np.sort(rng.choice(src, min(cpu_sources, len(src)), replace=False))
    t_cpu = time.perf_counter()
    X, ref_its = R.ppr_batched(sp.A, sample)
    t_cpu = time.perf_counter() - t_cpu
    sub = links[:, np.isin(links[0], sample)]
    ref_sc, _ = R.ppr_scores(sp.A, sub)
    got = sc.numpy()[np.isin(links[0], sample)]
    ppr["cpu_restatement"] = {"sources": int(len(sample)), "seconds": round(t_cpu, 3),
                              "scaled_to_all_sources_s": round(t_cpu * len(src) / len(sample), 2),
                              "threads": torch.get_num_threads()}
    ppr["max_rel_diff_vs_restatement"] = float(np.max(np.abs(got - ref_sc) / np.maximum(np.abs(ref_sc), 1e-30)))
    ppr["speedup_vs_cpu_restatement"] = round(ppr["cpu_restatement"]["scaled_to_all_sources_s"] / t, 1)
    out["PPR"] = ppr
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "heuristics_probe.json"))
    ap.add_argument("--cpu-sources", type=int, default=64)
    ap.add_argument("--datasets", nargs="+", default=["usair", "router", "cora", "pubmed"])
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128, 256, 512, 1024])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "datasets": {}}
    for name in args.datasets:
        r = probe(name, args.cpu_sources, args.widths)
        res["datasets"][name] = r
        print(name, json.dumps({k: r[k] for k in ("CN", "AA", "PPR")}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
