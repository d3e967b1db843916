"""Masked-sketch probe -> profiles/sketch_mask_probe.json.

PubMed (seed-0 train split, hops 2, num_perm 128, hll_p 8), WARMUP calls and then REPEATS timed ones of
`SketchGraph.features` as the caller sees it (host id check, upload, the pairs kernel, a device synchronise), on
three lists of 164 000 links:
  random      §24's list, 164 000 random pairs (a handful of them stored entries)
  entries     stored entries of the train graph only, taken cyclically: every link masked on both sides
  non_edges   the random list with its stored entries replaced: no link masked
each unmasked (the path of `mask=False`, §24's) and masked; the numpy restatements of both on this machine's CPUs
(tests/sketch_reference.py, tests/sketch_mask_reference.py), with a check that the HIP outputs equal them to the bit;
and the bytes the masked kernel is modelled to read: per masked endpoint deg·hops·(4P + m) for the neighbours' rows
and 4P + m for its own hop 0, per other endpoint (hops + 1)·(4P + m).
USAir and Cora (seed-0 splits, no node features): test AUC of `run_buddy` unmasked and masked, and of CN.

    python tools/sketch_mask_probe.py [--out profiles/sketch_mask_probe.json] [--epochs 50] [--quick]
    python tools/sketch_mask_probe.py --kernel-trace <rocprofv3 kernel_trace.csv of a --quick run> [--out ...]

`--quick` runs only the HIP timings, in the fixed order PHASES, for a kernel trace of its own
(`rocprofv3 --kernel-trace --stats -- python tools/sketch_mask_probe.py --quick`); `--kernel-trace` reads that trace,
takes the last REPEATS dispatches of every phase and adds their median to the JSON written before.
"""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))

HOPS, P, HLL_P = 2, 128, 8
WARMUP, REPEATS = 3, 20
MANY = 164000
PHASES = [(name, mask) for name in ("random", "entries", "non_edges") for mask in (False, True)]
ROW_BYTES = 4 * P + (1 << HLL_P)
# The rate DESIGN.md §24 ("Bound and measurement") compares its kernels with: MI355X_MICROARCH.md, "Indexed rows:
# gather into LDS", uniformly random rows of a 38 MB table served by the Infinity Cache, 8.6 TB/s chip-wide.  A
# reference rate, not a bound: the rows read here are degree-biased, not uniform, and PubMed's tables (45 MB over
# three hops) are partly served by the L2s.
RANDOM_ROW_RATE = 8.6e12
RANDOM_ROW_RATE_NOTE = ("MI355X_MICROARCH.md, 'Indexed rows: gather into LDS': uniformly random rows of a 38 MB table, "
                        "the rate DESIGN.md §24 compares with; a reference rate, not a bound (these rows are "
                        "degree-biased, not uniformly random)")


def gpu_times(fn, warmup=WARMUP, repeats=REPEATS):
    import torch

    ts = []
    for k in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(time.perf_counter() - t0)
    return {"median_s": round(float(np.median(ts)), 7), "min_s": round(min(ts), 7), "max_s": round(max(ts), 7),
            "repeats": repeats}


def link_lists(sp):
    """{'random', 'entries', 'non_edges'}: int64 [2, MANY] each, and how many entries of A each holds"""
    A, n = sp.A.tocsr(), sp.num_nodes
    rng = np.random.default_rng(0)
    random = rng.integers(0, n, size=(2, MANY)).astype(np.int64)
    coo = A.tocoo()
    at = np.arange(MANY) % A.nnz
    entries = np.stack([coo.row[at], coo.col[at]]).astype(np.int64)
    non_edges = random.copy()
    while True:
        hit = np.nonzero((np.asarray(A[non_edges[0], non_edges[1]]).reshape(-1) != 0)
                         | (np.asarray(A[non_edges[1], non_edges[0]]).reshape(-1) != 0))[0]
        if not len(hit):
            break
        non_edges[:, hit] = rng.integers(0, n, size=(2, len(hit)))
    return {"random": random, "entries": entries, "non_edges": non_edges}


def modelled_bytes(A, links):
    """(masked endpoints, bytes the masked kernel reads for `links` by the model in the module docstring)"""
    deg = np.diff(A.indptr)
    u, v = links
    su = np.asarray(A[u, v]).reshape(-1) != 0
    sv = np.asarray(A[v, u]).reshape(-1) != 0
    walked = int(deg[u][su].sum() + deg[v][sv].sum())
    masked = int(su.sum() + sv.sum())
    plain = 2 * links.shape[1] - masked
    return masked, walked * HOPS * ROW_BYTES + masked * ROW_BYTES + plain * (HOPS + 1) * ROW_BYTES + walked * 4


def pubmed(quick):
    import torch

    import sketch_mask_reference as MR
    import sketch_reference as R
    from heuristics_probe import split_of
    from s3grl_amd import sketch as S

    sp = split_of("pubmed")
    A = S.check_graph(sp.A)
    lists = link_lists(sp)
    out = {"num_nodes": sp.num_nodes, "nnz": int(A.nnz), "hops": HOPS, "num_perm": P, "hll_p": HLL_P,
           "links": MANY, "row_bytes": ROW_BYTES, "max_degree": int(np.diff(A.indptr).max()),
           "csr_bytes_kept": int((sp.num_nodes + 1) * 8 + A.nnz * 4), "lists": {}, "features": {}}
    sk = S.SketchGraph(A, HOPS, P, HLL_P)
    for name, links in lists.items():
        masked, nbytes = modelled_bytes(A, links)
        deg = np.diff(A.indptr)
        out["lists"][name] = {"masked_endpoints": masked, "modelled_bytes_masked": nbytes,
                              "modelled_bytes_unmasked": int(2 * MANY * (HOPS + 1) * ROW_BYTES),
                              "mean_endpoint_degree": round(float(deg[links].mean()), 2)}
    for name, mask in PHASES:
        key = f"{name}_{'masked' if mask else 'unmasked'}"
        out["features"][key] = gpu_times(lambda: sk.features(lists[name], mask=mask))
        print(key, out["features"][key], flush=True)
    f = out["features"]
    out["ratios"] = {"masked_random_over_unmasked_random": round(f["random_masked"]["median_s"] / f["random_unmasked"]["median_s"], 3),
                     "masked_non_edges_over_unmasked_random": round(f["non_edges_masked"]["median_s"] / f["random_unmasked"]["median_s"], 3),
                     "masked_entries_over_unmasked_entries": round(f["entries_masked"]["median_s"] / f["entries_unmasked"]["median_s"], 3),
                     "masked_entries_over_masked_non_edges": round(f["entries_masked"]["median_s"] / f["non_edges_masked"]["median_s"], 3)}
    if quick:
        sk.close()
        return out
    # the numpy restatements on the CPUs, and that the HIP outputs equal them
    t0 = time.perf_counter()
    mh, hl = R.sketches(A, HOPS, P, HLL_P, 0)
    out["numpy"] = {"build_s": round(time.perf_counter() - t0, 4), "threads": torch.get_num_threads()}
    equal = True
    for name, links in lists.items():
        t0 = time.perf_counter()
        plain = R.link_outputs(mh, hl, links, HLL_P)["features"]
        t1 = time.perf_counter()
        masked = MR.masked_link_outputs(A, mh, hl, links, HLL_P)["features"]
        t2 = time.perf_counter()
        out["numpy"][f"{name}_unmasked_s"], out["numpy"][f"{name}_masked_s"] = round(t1 - t0, 4), round(t2 - t1, 4)
        equal = equal and np.array_equal(sk.features(links).cpu().numpy().view(np.uint32), plain.view(np.uint32)) \
            and np.array_equal(sk.features(links, mask=True).cpu().numpy().view(np.uint32), masked.view(np.uint32))
        out["lists"][name]["rows_changed_by_masking"] = int((plain.view(np.uint32) != masked.view(np.uint32)).any(axis=1).sum())
    out["hip_bit_equal_to_numpy"] = bool(equal)
    sk.close()
    return out


def auc_rows(name, epochs):
    from heuristics_probe import split_of
    from s3grl_amd import heuristics as H
    from s3grl_amd import sketch as S

    sp = split_of(name)
    kw = dict(hops=HOPS, epochs=epochs, lr=0.01, seed=1)

    def both(r):
        return {k: [round(v[0], 6), round(v[1], 6)] for k, v in r.items()}

    return {"num_nodes": sp.num_nodes, "epochs": epochs, "run_buddy_unmasked": both(S.run_buddy(sp, **kw)),
            "run_buddy_masked": both(S.run_buddy(sp, mask=True, **kw)), "CN": both(H.run_heuristic(sp, "CN"))}


def kernel_times(trace):
    """Median kernel time per phase from a rocprofv3 kernel trace of a --quick run."""
    with open(trace, newline="") as f:
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    runs = [(e - b, "masked" in k) for b, e, k in rows if "pairs_kernel" in k]
    per = WARMUP + REPEATS
    if len(runs) != per * len(PHASES):
        raise SystemExit(f"expected {per * len(PHASES)} pairs-kernel dispatches, found {len(runs)}")
    out = {}
    for at, (name, mask) in enumerate(PHASES):
        chunk = runs[at * per:(at + 1) * per]
        assert all(m == mask for _, m in chunk), (name, mask)
        ns = [d for d, _ in chunk[WARMUP:]]
        out[f"{name}_{'masked' if mask else 'unmasked'}"] = {"median_us": round(float(np.median(ns)) / 1e3, 2),
                                                            "min_us": round(min(ns) / 1e3, 2),
                                                            "max_us": round(max(ns) / 1e3, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "sketch_mask_probe.json"))
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-trace")
    args = ap.parse_args()
    if args.kernel_trace:
        res = json.loads(Path(args.out).read_text())
        kt = res["pubmed"]["kernel"] = kernel_times(args.kernel_trace)
        res["pubmed"]["kernel_source"] = ("a separate process: `rocprofv3 --kernel-trace --stats -- python "
                                          "tools/sketch_mask_probe.py --quick`, the same calls in the same order; "
                                          "the wall times under `features` are from the untraced full run")
        for key, row in kt.items():
            name, kind = key.rsplit("_", 1)
            nbytes = res["pubmed"]["lists"][name][f"modelled_bytes_{kind}"]
            row["modelled_TB_per_s"] = round(nbytes / (row["median_us"] * 1e-6) / 1e12, 3)
            row["share_of_random_row_rate"] = round(nbytes / (row["median_us"] * 1e-6) / RANDOM_ROW_RATE, 3)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(kt))
        return
    import torch

    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS,
           "random_row_rate_B_per_s": RANDOM_ROW_RATE, "random_row_rate_note": RANDOM_ROW_RATE_NOTE}
    res["pubmed"] = pubmed(args.quick)
    print("pubmed", json.dumps(res["pubmed"]), flush=True)
    if not args.quick:
        res["auc"] = {}
        for name in ("usair", "cora"):
            res["auc"][name] = auc_rows(name, args.epochs)
            print(name, json.dumps(res["auc"][name]), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
        print("wrote", args.out)


if __name__ == "__main__":
    main()
