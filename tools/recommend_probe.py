"""Link recommendation probe -> profiles/recommend_probe.json.

For PubMed and USAir, every node a source, hops = 2, k = 10:
(a) candidate enumeration (s3grl_candidates_count + _fill, from the sources on the device to seg_ptr / cand on the
    device) next to scipy's (A @ A) minus A minus I on the CPUs of the same machine (scipy's sparse product runs on one
    thread whatever the machine has); the two results are compared;
(b) `segment_topk` on the common-neighbour scores of those candidates next to the plain torch formulation on the same
    GPU: a stable sort by score, a stable sort by segment id, a slice; the two results are compared;
(c) the whole `recommend` with `SignScorer` (seeded, untrained SIGNNet of the workload's own mode / num_hops / sign_k:
    the time does not depend on the weights) and with `HeuristicScorer("CN")`, split into enumeration, scoring and
    top-K (each phase waited for).
Every time is a host clock around a call that ends with the device idle, the median of --repeats calls after --warmup.

    python tools/recommend_probe.py [--out profiles/recommend_probe.json] [--repeats 10] [--warmup 2]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import scipy.sparse as ssp
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from s3grl_amd import recommend as R, workloads  # noqa: E402
from s3grl_amd.engine import default_engine  # noqa: E402
from s3grl_amd.heuristics import Heuristics  # noqa: E402
from s3grl_amd.signnet import SIGNNetTrainer  # noqa: E402

K, HOPS = 10, 2


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


def scipy_candidates(A):
    B = ssp.csr_matrix((np.ones(A.nnz, dtype=np.int32), A.indices, A.indptr), shape=A.shape)
    P = (B @ B).tocsr()
    P.data[:] = 1
    P = P - P.multiply(B + ssp.identity(A.shape[0], dtype=np.int32, format="csr"))
    P.eliminate_zeros()
    P.sort_indices()
    return P


def torch_topk(scores, seg_ptr, cand, k):
    S, P = seg_ptr.numel() - 1, scores.numel()
    seg = torch.repeat_interleave(torch.arange(S, device=scores.device), seg_ptr.diff(), output_size=P)
    o1 = torch.sort(scores, descending=True, stable=True).indices
    o2 = torch.sort(seg[o1], stable=True).indices
    order = o1[o2]
    rank = torch.arange(P, device=scores.device) - seg_ptr[seg[order]]
    keep = rank < k
    nodes = torch.full((S, k), -1, dtype=torch.int32, device=scores.device)
    top = torch.full((S, k), float("-inf"), dtype=torch.float32, device=scores.device)
    nodes[seg[order][keep], rank[keep]] = cand[order][keep]
    top[seg[order][keep], rank[keep]] = scores[order][keep]
    return nodes, top


class Phases:
    """Where one `recommend` call spends its time: while active, the module's count / fill (enumeration) and top-K
    steps and the scorer run between two device synchronisations and their host seconds are summed.  What is left of
    the total is the host code between them (the prefix read, cutting chunks, building the pair list)."""

    def __init__(self, scorer):
        self.seconds = {"enumerate_s": 0.0, "score_s": 0.0, "topk_s": 0.0}
        self.scorer = self.timed(scorer, "score_s")

    def timed(self, fn, key):
        def run(*args, **kwargs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn(*args, **kwargs)
            torch.cuda.synchronize()
            self.seconds[key] += time.perf_counter() - t0
            return res
        return run

    def __enter__(self):
        self.saved = (R._count, R._fill, R._topk_into)
        R._count, R._fill = self.timed(R._count, "enumerate_s"), self.timed(R._fill, "enumerate_s")
        R._topk_into = self.timed(R._topk_into, "topk_s")
        return self

    def __exit__(self, *exc):
        R._count, R._fill, R._topk_into = self.saved


def probe(name, chunk_pairs, warmup, repeats):
    eng = default_engine("cuda:0")
    w = workloads.make(name)
    n = w.A.shape[0]
    G, f, h = eng.graph(w.A), eng.features(w.X), Heuristics(w.A, device="cuda:0")
    sources = torch.arange(n, dtype=torch.int32, device=eng.device)
    out = {"workload": name, "num_nodes": n, "nnz": int(w.A.nnz), "k": K, "hops": HOPS, "layout": R.layout(n, HOPS)}
    # (a)
    seg_ptr, cand = R.candidates(G, sources, HOPS)
    out["pairs"] = int(cand.numel())
    out["longest_segment"] = int(seg_ptr.diff().max())
    out["candidates_s"] = median_s(lambda: R.candidates(G, sources, HOPS), warmup, repeats)
    t = []
    for i in range(warmup + repeats):          # the same warm-up and repeats as the kernels get
        t0 = time.perf_counter()
        P = scipy_candidates(w.A)
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    out["scipy_s"] = statistics.median(t)
    out["same_as_scipy"] = bool(np.array_equal(P.indptr, seg_ptr.cpu().numpy()) and
                                np.array_equal(P.indices, cand.cpu().numpy()))
    out["candidates_speedup_vs_scipy"] = out["scipy_s"] / out["candidates_s"]
    # (b)
    pairs = torch.stack([torch.repeat_interleave(sources.long(), seg_ptr.diff()), cand.long()])
    scores = h.cn(pairs)
    top = R.segment_topk(scores, seg_ptr, cand, K, engine=eng)
    tn, ts = torch_topk(scores, seg_ptr, cand, K)
    out["same_as_torch"] = bool(torch.equal(top.nodes, tn) and torch.equal(top.scores, ts))
    out["segment_topk_s"] = median_s(lambda: R.segment_topk(scores, seg_ptr, cand, K, engine=eng), warmup, repeats)
    out["torch_two_sorts_s"] = median_s(lambda: torch_topk(scores, seg_ptr, cand, K), warmup, repeats)
    out["segment_topk_speedup_vs_torch"] = out["torch_two_sorts_s"] / out["segment_topk_s"]
    del pairs
    # (c)
    net = SIGNNetTrainer((w.sign_k + 1) * (1 + w.X.shape[1]), hidden=256, seed=0, device="cuda:0")
    scorers = {"sign": R.SignScorer(eng, G, f, net, mode=w.mode, num_hops=w.num_hops, sign_k=w.sign_k),
               "cn": R.HeuristicScorer(h, "CN")}
    out["chunk_pairs"] = chunk_pairs
    for key, scorer in scorers.items():
        runs = []
        for i in range(warmup + max(3, repeats // 2)):
            with Phases(scorer) as ph:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                R.recommend(G, sources, ph.scorer, k=K, hops=HOPS, chunk_pairs=chunk_pairs)
                torch.cuda.synchronize()
                ph.seconds["total_s"] = time.perf_counter() - t0
            if i >= warmup:
                runs.append(ph.seconds)
        out[f"recommend_{key}"] = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    out["sign_scorer"] = {"mode": w.mode, "num_hops": w.num_hops, "sign_k": w.sign_k, "features": int(w.X.shape[1])}
    net.close()
    h.close()
    G.close()
    f.close()
    eng.trim()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "recommend_probe.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup, "graphs": []}
    for name, chunk in (("usair_pos_k2", 1 << 20), ("pubmed_pos_k3", 1 << 18)):
        r = probe(name, chunk, args.warmup, args.repeats)
        res["graphs"].append(r)
        print(json.dumps(r), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
