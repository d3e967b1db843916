"""SoP balls probe -> profiles/sop_balls_probe.json.

What `Sop.run` costs where a link's scalar ball does not fit LDS and is formed in an HBM workspace (class 3), and
that the flavour costs nothing where no link needs it.  Times are device-event times (`Engine.timings` with profiling
on) of one `Sop.run` over the whole list, after one warm-up run.

  (a) `pubmed_sop_k3` (no class-3 link): sop_run_ms of five runs.  `--tree PATH` measures another checkout's engine
      (the parent commit's, built there) with the same code; `--parent-json FILE` copies such a record in beside this
      tree's, so that the two sets of five stand side by side; `--earlier-json FILE...` appends part-(a) records of
      earlier processes (either tree, alternating) as they are: the process-to-process drift.
  (b) the `collab_pos_k3` graph, SoP at sign_k = 3 on all 1 000 000 links: class counts, sop_run_ms, the time of the
      class-3 launches alone, and the largest rel_err (the test suite's: row-norm floored, ATOL 1e-10) over the 50
      class-3 links with the largest ball bound plus 250 random class-3 links, against rows of Â^i formed by sparse
      vector-matrix products in fp64.
  (c) the PubMed split at sign_k = 6 and 8, all links: class counts and sop_run_ms.

    python tools/sop_balls_probe.py [--parts abc] [--out profiles/sop_balls_probe.json] [--tree PATH] [--parent-json FILE]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import scipy.sparse as ssp
import torch

REPO = Path(__file__).resolve().parent.parent
ATOL = 1e-10


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=-1, keepdims=True))
    return float(np.max(np.clip(np.abs(got - ref) - ATOL, 0, None) / np.maximum(scale, 1e-30)))


def sop_rows_sparse(A, X, links, K):
    """rows [2L, K+1, 1+F] in fp64: row a of Â^i as a sparse vector, i products from e_a, times X, with the
    term of column b taken out; Â^i[a,a] prepended.  links [2, L]."""
    A = ssp.csr_matrix(A)
    n = A.shape[0]
    deg = np.diff(A.indptr).astype(np.float64)
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1.0)), 0.0)
    D = ssp.diags(dinv)
    op = (D @ (A != 0).astype(np.float64) @ D).tocsr()
    X = np.asarray(X, dtype=np.float64)
    F = X.shape[1]
    L = links.shape[1]
    cache = {}

    def power_rows(a):
        """per operator: (dense row of Â^i, the row times X) — shared by every link of endpoint a"""
        if a not in cache:
            v = ssp.csr_matrix(([1.0], ([0], [a])), shape=(1, n))
            out = []
            for _ in range(K):
                v = (v @ op).tocsr()
                out.append((v, np.asarray(v @ X).ravel()))
            cache[a] = out
        return cache[a]

    rows = np.empty((2 * L, K + 1, 1 + F))
    for l in range(L):
        s, d = int(links[0, l]), int(links[1, l])
        for e, (a, b) in enumerate(((s, d), (d, s))):
            rows[2 * l + e, 0, 0] = 1.0
            rows[2 * l + e, 0, 1:] = X[a]
            for i, (v, vx) in enumerate(power_rows(a)):
                rows[2 * l + e, i + 1, 0] = v[0, a]
                # column b zeroed = its term taken out of the whole row's product (fp64: 1e-16 of the row)
                rows[2 * l + e, i + 1, 1:] = vx - v[0, b] * X[b]
    return rows


class Runner:
    """one graph, one feature matrix, one link list on the device"""

    def __init__(self, eng, engine_mod, A, X, links):
        self.eng, self.engine_mod = eng, engine_mod
        self.G = eng.graph(A)
        self.x = eng.features(np.ascontiguousarray(X, dtype=np.float32))
        self.links = eng.links(links)
        self.out = None

    def timed_runs(self, K, runs):
        """-> (list of per-run timings dicts, class counts or None, rows of the last run)"""
        sop = self.engine_mod.Sop(self.eng, self.G, self.x, K)
        try:
            L = int(self.links.shape[0])
            shape = (2 * L, K + 1, sop.F + 1)
            if self.out is None or tuple(self.out.shape) != shape:
                self.out = None
                self.out = torch.empty(shape, dtype=torch.float32, device=self.eng.device)
            sop.run(self.links, self.out)          # warm-up: code objects, arena
            torch.cuda.synchronize()
            recs = []
            for _ in range(runs):
                self.eng.set_profiling(True)
                sop.run(self.links, self.out)
                tm = self.eng.timings()
                self.eng.set_profiling(False)
                recs.append({"sop_run_ms": tm["sop_run_ms"], "sop_rows_ms": tm["sop_rows_ms"],
                             "sop_hbm_balls_ms": tm.get("sop_hbm_balls_ms")})
            cls = getattr(sop, "last_class_links", None)
        finally:
            sop.close()
        return recs, (list(cls) if cls is not None else None), self.out

    def close(self):
        self.out = None
        self.G.close()


def spread(vals):
    return {"runs": vals, "median": statistics.median(vals), "min": min(vals), "max": max(vals)}


def part_a(eng, engine_mod, workloads):
    w = workloads.make("pubmed_sop_k3")
    links, _ = w.split.all_links()
    r = Runner(eng, engine_mod, w.A, w.X, links)
    recs, cls, _ = r.timed_runs(3, 5)
    r.close()
    return {"workload": "pubmed_sop_k3", "links": int(links.shape[1]), "class_links": cls,
            "sop_run_ms": spread([x["sop_run_ms"] for x in recs])}


def part_b(eng, engine_mod, workloads, sample=None):
    w = workloads.make("collab_pos_k3")
    links, _ = w.split.all_links()
    if sample:
        links = links[:, :sample]
    K = 3
    n = w.split.num_nodes
    lay = engine_mod.sop_layout(n, K)
    r = Runner(eng, engine_mod, w.A, w.X, links)
    recs, cls, rows = r.timed_runs(K, 3)
    deg = np.diff(w.A.indptr)
    bound = deg[links[0]] + deg[links[1]] + 2
    big = np.flatnonzero(bound > lay["nodes_lds"])
    rng = np.random.default_rng(0)
    top = big[np.argsort(-bound[big], kind="stable")[:50]]
    rest = np.setdiff1d(big, top)
    pick = np.concatenate([top, rng.choice(rest, min(250, len(rest)), replace=False)]) if len(big) else big
    err = None
    if len(pick):
        idx = torch.as_tensor(np.stack([2 * pick, 2 * pick + 1], 1).reshape(-1), device=rows.device)
        got = rows[idx].cpu().numpy()
        ref = sop_rows_sparse(w.A, w.X.astype(np.float32).astype(np.float64), links[:, pick], K)
        err = rel_err(got, ref)
    r.close()
    return {"graph": "collab_pos_k3", "num_nodes": int(n), "max_degree": int(deg.max()), "sign_k": K,
            "links": int(links.shape[1]), "whole_list": sample is None, "nodes_lds": lay["nodes_lds"],
            "links_over_the_bound_counted_on_cpu": int(len(big)), "largest_bound": int(bound.max()),
            "class_links": cls,
            "sop_run_ms": spread([x["sop_run_ms"] for x in recs]),
            "class3_launches_ms": spread([x["sop_hbm_balls_ms"] for x in recs]),
            "sop_rows_ms": spread([x["sop_rows_ms"] for x in recs]),
            "checked_class3_links": int(len(pick)), "max_rel_err_of_checked_links": err}


def part_c(eng, engine_mod, workloads):
    w = workloads.make("pubmed_sop_k3")
    links, _ = w.split.all_links()
    r = Runner(eng, engine_mod, w.A, w.X, links)
    out = []
    for K in (6, 8):
        recs, cls, _ = r.timed_runs(K, 3)
        out.append({"graph": "pubmed_sop_k3", "sign_k": K, "links": int(links.shape[1]),
                    "nodes_lds": engine_mod.sop_layout(w.split.num_nodes, K)["nodes_lds"], "class_links": cls,
                    "sop_run_ms": spread([x["sop_run_ms"] for x in recs]),
                    "class3_launches_ms": spread([x["sop_hbm_balls_ms"] for x in recs])})
    r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--out", default=str(REPO / "profiles" / "sop_balls_probe.json"))
    ap.add_argument("--tree", default=str(REPO), help="the checkout whose engine is measured")
    ap.add_argument("--parent-json", default=None, help="a part-(a) record of the parent commit to place beside this one")
    ap.add_argument("--earlier-json", nargs="*", default=[], help="part-(a) records of earlier processes, kept as they are")
    ap.add_argument("--collab-sample", type=int, default=None, help="part (b) on the first N links only")
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    from s3grl_amd import engine as engine_mod, workloads  # noqa: E402

    assert torch.cuda.is_available(), "the probe measures on the GPU"
    eng = engine_mod.Engine("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "tree": "this" if args.tree == str(REPO) else "other",
           "timing": "HIP events around s3grl_sop_run's launches (Engine.timings), one run each, after one warm-up run"}
    if "a" in args.parts:
        res["a_pubmed_sop_k3"] = {"this_commit": part_a(eng, engine_mod, workloads)}
        if args.parent_json:
            parent = json.loads(Path(args.parent_json).read_text())["a_pubmed_sop_k3"]["this_commit"]
            res["a_pubmed_sop_k3"]["parent_commit"] = parent
            med = res["a_pubmed_sop_k3"]["this_commit"]["sop_run_ms"]["median"]
            res["a_pubmed_sop_k3"]["median_inside_parent_spread"] = \
                parent["sop_run_ms"]["min"] <= med <= parent["sop_run_ms"]["max"]
            res["a_pubmed_sop_k3"]["median_not_above_parent_max"] = med <= parent["sop_run_ms"]["max"]
        for f in args.earlier_json:
            rec = json.loads(Path(f).read_text())
            res["a_pubmed_sop_k3"].setdefault("earlier_processes", []).append(
                {"tree": "this commit" if rec["tree"] == "this" else "parent commit",
                 "sop_run_ms": rec["a_pubmed_sop_k3"]["this_commit"]["sop_run_ms"]})
    if "b" in args.parts:
        res["b_collab_sign_k3"] = part_b(eng, engine_mod, workloads, args.collab_sample)
    if "c" in args.parts:
        res["c_pubmed_sign_k_6_8"] = part_c(eng, engine_mod, workloads)
    eng.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
