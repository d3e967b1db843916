"""Labelled enclosing subgraphs (s3grl_amd.seal) on the GPU: links/s of the SEAL configs of the reference's
paper runs, and the CPU restatement (tests/seal_reference.py, reference-structured: scipy shortest_path per
link) on a sample of links on one core.

    python tools/seal_probe.py --out DIR            # one JSON line per config, also DIR/seal_probe.json
    python tools/seal_probe.py --no-cpu             # GPU part only (run it under rocprofv3 --kernel-trace --stats)

Configs: USAir 2-hop drnl (table_2), Cora 3-hop drnl and de (profiling_attr), all 164 000 PubMed links at
3 hops drnl in chunks of --chunk links.  Link lists: s3grl_amd.workloads.edge_split (seed 0) — train
positives both directions, negatives, valid / test.
"""
import argparse
import json
import os
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

CONFIGS = [("usair", 2, "drnl"), ("cora", 3, "drnl"), ("cora", 3, "de"), ("pubmed", 3, "drnl")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-sample", type=int, default=200)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    from s3grl_amd import workloads as W
    from s3grl_amd.engine import Engine
    from s3grl_amd.seal import labelled_subgraphs

    if not torch.cuda.is_available():
        sys.exit("seal_probe needs the MI355X")
    eng = Engine("cuda:0")
    results = []
    for name, hops, label in CONFIGS:
        n, e = W.load_topology(name)
        sp = W.edge_split(n, e, seed=0)
        li, _ = sp.all_links()
        G = eng.graph(sp.A)
        links = eng.links(li)
        L = links.shape[0]

        def once():
            tot_n = tot_e = 0
            for a in range(0, L, args.chunk):
                s = labelled_subgraphs(eng, G, links[a:a + args.chunk], num_hops=hops, node_label=label)
                tot_n += s.nodes.numel()
                tot_e += s.src.numel()
                del s
            torch.cuda.synchronize()
            return tot_n, tot_e

        once()   # warm-up: code objects, arena
        times = []
        for _ in range(args.repeats):
            t = time.perf_counter()
            tot_n, tot_e = once()
            times.append(time.perf_counter() - t)
        best = min(times)
        r = {"config": f"{name} {hops}-hop {label}", "links": L, "chunk": args.chunk, "nodes": tot_n,
             "edges": tot_e, "gpu_s": [round(x, 4) for x in times], "gpu_links_per_s": round(L / best, 1)}
        if not args.no_cpu:
            from seal_reference import label_subgraph

            torch.set_num_threads(1)
            s = labelled_subgraphs(eng, G, links[:args.cpu_sample], num_hops=hops, node_label=label)
            ptr = s.node_ptr.cpu().numpy()
            nodes = s.nodes.cpu().numpy()
            dists = s.dists.cpu().numpy()
            t = time.perf_counter()
            for i in range(len(ptr) - 1):
                label_subgraph(sp.A, nodes[ptr[i]:ptr[i + 1]], dists[ptr[i]:ptr[i + 1]], label)
            dt = time.perf_counter() - t
            r["cpu_restatement_links_per_s_one_core"] = round((len(ptr) - 1) / dt, 1)
            r["cpu_what"] = ("tests/seal_reference.py on the first %d links (labels and edges from the node lists; "
                             "the BFS extraction itself not included), one core" % (len(ptr) - 1))
        G.close()
        print(json.dumps(r), flush=True)
        results.append(r)
    eng.close()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        Path(args.out, "seal_probe.json").write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
