"""RA / Jaccard / PA / Katz probe -> profiles/heuristics_more_probe.json.

For USAir, Router (tests/golden/router_edges.txt), Cora and PubMed, each on its seed-0 train split (the splits of
tools/heuristics_probe.py, so the numbers stand next to §11's):
  * val and test AUC / AP of RA, JACCARD, PA and KATZ through `run_heuristic`, and KATZ at max_len 7;
  * GPU wall time of each index over the four full val/test lists (host clock around the call, ending in the scores'
    read-back; a warm-up call first), Katz over every distinct source of the four lists at once, at the default
    (β 0.005, max_len 3) and at max_len 7;
  * Katz at block widths 64 .. 1024 next to the default width;
  * the CPU restatement (tests/heuristics_more_reference.py) of the same lists on this process's threads, and the
    largest difference between the two in fp32 ulps of the restatement.

    python tools/heuristics_more_probe.py [--out profiles/heuristics_more_probe.json] [--datasets ...]
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

import heuristics_more_reference as M  # noqa: E402
from heuristics_probe import split_of, timed  # noqa: E402
from s3grl_amd import heuristics as H  # noqa: E402

LOCAL = (("RA", "ra", M.ra), ("JACCARD", "jaccard", M.jaccard), ("PA", "pa", M.pa))


def cpu_timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def ulps(got, ref):
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / M.ulp32(ref)
    return float(err.max()) if err.size else 0.0


def row(sp, name, **kw):
    return {k: [round(v[0], 6), round(v[1], 6)] for k, v in H.run_heuristic(sp, name, **kw).items()}


def probe(name, widths):
    sp = split_of(name)
    lists = [sp.links["valid"][0], sp.links["valid"][1], sp.links["test"][0], sp.links["test"][1]]
    links = np.concatenate(lists, axis=1)
    out = {"num_nodes": sp.num_nodes, "nnz": int(sp.A.nnz), "links": int(links.shape[1]),
           "distinct_sources": int(len(np.unique(links[0]))), "max_column_entries": M.max_column_entries(sp.A)}
    h = H.Heuristics(sp.A)
    for kind, method, ref_fn in LOCAL:
        fn = getattr(h, method)
        fn(links)
        sc, t = timed(lambda: fn(links))
        ref, t_cpu = cpu_timed(lambda: ref_fn(sp.A, links))
        out[kind] = {"gpu_s": round(t, 6), "cpu_restatement_s": round(t_cpu, 4), **row(sp, kind),
                     "max_ulp_diff_vs_restatement": ulps(sc.numpy(), ref)}
    katz = {}
    for label, kw in (("default", dict(beta=0.005, max_len=3)), ("max_len_7", dict(beta=0.005, max_len=7))):
        h.katz(links, **kw)
        sc, t = timed(lambda: h.katz(links, **kw))
        ref, t_cpu = cpu_timed(lambda: M.katz(sp.A, links, **kw))
        katz[label] = {**kw, "gpu_s": round(t, 6), "cpu_restatement_s": round(t_cpu, 4), **row(sp, "KATZ", **kw),
                       "max_ulp_diff_vs_restatement": ulps(sc.numpy(), ref),
                       "speedup_vs_cpu_restatement": round(t_cpu / t, 1), "widths": {}}
        for bw in widths:
            sw, tw = timed(lambda: h.katz(links, block_width=bw, **kw))
            katz[label]["widths"][str(bw)] = {"gpu_s": round(tw, 6), "bit_equal_to_default": bool(torch.equal(sw, sc))}
    out["KATZ"] = katz
    h.close()
    out["cpu_threads"] = torch.get_num_threads()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "heuristics_more_probe.json"))
    ap.add_argument("--datasets", nargs="+", default=["usair", "router", "cora", "pubmed"])
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128, 256, 512, 1024])
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "datasets": {}}
    for name in args.datasets:
        r = probe(name, args.widths)
        res["datasets"][name] = r
        print(name, json.dumps({k: r[k] for k in ("RA", "JACCARD", "PA", "KATZ")}), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
