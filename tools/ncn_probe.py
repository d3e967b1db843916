"""NCN probe -> profiles/ncn_probe.json.

PubMed (seed-0 train graph), H = 256, on two lists of 164 000 links:
  random    164 000 random pairs: nearly every list is empty
  entries   164 000 stored entries of the train graph, taken cyclically: degree-biased, far longer lists
WARMUP calls and then REPEATS timed ones, medians reported, every timed call ending in a device synchronise, of
  build     `CommonNeighbours` from the device CSR and device links (count, scan, fill, the host's id checks)
  transpose the stable sort behind `.t_ptr` / `.t_link`
  forward   `s3grl_segment_sum` over the lists (what `common_neighbour_sum` runs)
  backward  `s3grl_segment_sum` over the transpose
against (a) plain torch on the same GPU, the way NCN's own code does it: sparse row products A[u] * A[v] and
`torch.sparse.mm` with Z for the forward, with the transposed mask and the upstream gradient for the backward; and
(b) the numpy restatement (tests/ncn_reference.py) on this machine's CPUs, with a check that the HIP outputs equal it
to the bit.  Modelled bytes: Σ|CN|·H·4 for the rows summed plus 4·(deg u + deg v) for the two rows' keys per link,
and the rate they imply beside the random-row gather rate of MI355X_MICROARCH.md.
USAir and Cora (seed-0 splits, no node features): test AUC / AP of `run_ncn` for use_cn True / False and mask True /
False, beside CN's and `run_mpgnn(split, "GCN")`'s on the same splits.

    python tools/ncn_probe.py [--out profiles/ncn_probe.json] [--epochs 50] [--quick]
    python tools/ncn_probe.py --kernel-trace <rocprofv3 kernel_trace.csv of a --quick run> [--out ...]

`--quick` skips the CPU restatement and the AUC rows and writes nothing, for a kernel trace of its own (`rocprofv3
--kernel-trace --stats -- python tools/ncn_probe.py --quick`); `--kernel-trace` reads that trace, takes the last
REPEATS dispatches of every phase and adds their median to the JSON written before.
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

H = 256
WARMUP, REPEATS = 3, 20
MANY = 164000
# MI355X_MICROARCH.md, "Indexed rows": random whole rows gathered into registers, each fetched once from a buffer far
# larger than the Infinity Cache, one wave per destination and 4 rows in flight per wave: 5.5-5.6 TB/s for 1 152-byte
# rows.  A reference rate, not a bound: Z here is 20 MB (it fits the Infinity Cache) and its rows are 1 024 bytes.
RANDOM_ROW_RATE = 5.5e12
RANDOM_ROW_RATE_NOTE = ("MI355X_MICROARCH.md, 'Indexed rows': random 1 152-byte rows gathered into registers, one wave "
                        "per destination, 4 rows in flight; a reference rate, not a bound (Z is 20 MB and degree-biased)")


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
    A, n = sp.A.tocsr(), sp.num_nodes
    rng = np.random.default_rng(0)
    coo = A.tocoo()
    at = np.arange(MANY) % A.nnz
    return {"random": rng.integers(0, n, size=(2, MANY)).astype(np.int64),
            "entries": np.stack([coo.row[at], coo.col[at]]).astype(np.int64)}


def torch_baseline(A, links, z, g):
    """NCN's own way in plain torch: the sparse rows A[u] and A[v], their elementwise product, and sparse x dense
    products with it.  Returns (times, forward, backward) or ({'not_measured': why}, None, None)."""
    import torch

    dev = z.device
    try:
        coo = A.tocoo()
        At = torch.sparse_coo_tensor(torch.as_tensor(np.stack([coo.row, coo.col])).to(dev),
                                     torch.ones(coo.nnz, device=dev), A.shape).coalesce()
        u, v = torch.as_tensor(links[0]).to(dev), torch.as_tensor(links[1]).to(dev)

        def build():
            return (At.index_select(0, u).coalesce() * At.index_select(0, v).coalesce()).coalesce()

        mask = build()
        mask_t = mask.t().coalesce()
        times = {"build": gpu_times(build), "forward": gpu_times(lambda: torch.sparse.mm(mask, z)),
                 "transpose": gpu_times(lambda: mask.t().coalesce()),
                 "backward": gpu_times(lambda: torch.sparse.mm(mask_t, g))}
        return times, torch.sparse.mm(mask, z), torch.sparse.mm(mask_t, g)
    except Exception as e:          # an operator this torch build lacks: said, not hidden
        return {"not_measured": f"{type(e).__name__}: {e}"[:300]}, None, None


def pubmed(quick):
    import torch

    import ncn_reference as R
    from heuristics_probe import split_of
    from s3grl_amd import ncn
    from s3grl_amd.heuristics import canonical_csr

    sp = split_of("pubmed")
    A = canonical_csr(sp.A)
    n, deg = sp.num_nodes, np.diff(A.indptr)
    g0 = ncn._TrainGraph(A)
    dev = g0.engine.device
    z_np = R.values((n, H), seed=1)
    z = torch.as_tensor(z_np).to(dev)
    out = {"num_nodes": n, "nnz": int(A.nnz), "H": H, "links": MANY, "max_degree": int(deg.max()),
           "z_bytes": int(z.numel() * 4), "lists": {}}
    for name, links in link_lists(sp).items():
        l_d = torch.as_tensor(links).to(dev)
        cn = ncn.CommonNeighbours(g0.csr(), l_d, False)
        total = int(cn.idx.numel())
        g_np = R.values((MANY, H), seed=2)
        g = torch.as_tensor(g_np).to(dev)
        row = {"sum_cn": total, "mean_cn": round(total / MANY, 3), "max_cn": int(cn.counts.max()),
               "mean_endpoint_degree": round(float(deg[links].mean()), 2),
               "max_links_per_node": int(cn.t_ptr.diff().max())}
        key_bytes = int(4 * (deg[links[0]].sum() + deg[links[1]].sum()))
        row["modelled_bytes"] = {"build": 2 * key_bytes, "forward": total * H * 4 + total * 4 + MANY * H * 4,
                                 "backward": total * H * 4 + total * 4 + n * H * 4,
                                 "note": "build: the two rows' keys per link, count and fill; forward / backward: "
                                         "Σ|CN|·H·4 gathered, the ids, and the output written"}

        def transpose():
            cn._t = None
            cn.t_link

        hip = {"build": gpu_times(lambda: ncn.CommonNeighbours(g0.csr(), l_d, False)),
               "transpose": gpu_times(transpose),
               "forward": gpu_times(lambda: ncn._segment_sum(z, cn.ptr, cn.idx, MANY)),
               "backward": gpu_times(lambda: ncn._segment_sum(g, cn.t_ptr, cn.t_link, n))}
        for k in ("build", "forward", "backward"):
            rate = row["modelled_bytes"][k] / hip[k]["median_s"]
            hip[k]["modelled_TB_per_s_wall"] = round(rate / 1e12, 4)
            hip[k]["share_of_random_row_rate"] = round(rate / RANDOM_ROW_RATE, 4)
        row["hip"] = hip
        print(name, "hip", json.dumps(hip), flush=True)
        fwd = ncn._segment_sum(z, cn.ptr, cn.idx, MANY)
        bwd = ncn._segment_sum(g, cn.t_ptr, cn.t_link, n)
        times, t_fwd, t_bwd = torch_baseline(A, links, z, g)
        row["torch_same_gpu"] = times
        if t_fwd is not None:
            row["torch_max_abs_difference"] = {"forward": float((t_fwd - fwd).abs().max()),
                                               "backward": float((t_bwd - bwd).abs().max())}
            row["hip_speedup_over_torch"] = {k: round(times[k]["median_s"] / hip[k]["median_s"], 2) for k in hip}
        print(name, "torch", json.dumps(times), flush=True)
        if not quick:
            t0 = time.perf_counter()
            ptr, idx = R.cn_lists(A, links, False)
            t1 = time.perf_counter()
            ref_f = R.segment_sum(z_np, ptr, idx)
            t2 = time.perf_counter()
            t_ptr, t_link = R.transpose(ptr, idx, n)
            t3 = time.perf_counter()
            ref_b = R.segment_sum(g_np, t_ptr, t_link)
            t4 = time.perf_counter()
            cpu = {"build": round(t1 - t0, 4), "forward": round(t2 - t1, 4), "transpose": round(t3 - t2, 4),
                   "backward": round(t4 - t3, 4)}
            row["numpy_cpu_s"] = cpu
            row["hip_speedup_over_numpy"] = {k: round(cpu[k] / hip[k]["median_s"], 1) for k in hip}
            same = (np.array_equal(cn.ptr.cpu().numpy(), ptr) and np.array_equal(cn.idx.cpu().numpy(), idx)
                    and np.array_equal(cn.t_link.cpu().numpy(), t_link)
                    and np.array_equal(fwd.cpu().numpy().view(np.uint32), ref_f.view(np.uint32))
                    and np.array_equal(bwd.cpu().numpy().view(np.uint32), ref_b.view(np.uint32)))
            row["hip_bit_equal_to_numpy"] = bool(same)
            print(name, "numpy", json.dumps(cpu), "bit equal", same, flush=True)
        out["lists"][name] = row
    return out


def auc_rows(name, epochs):
    from heuristics_probe import split_of
    from s3grl_amd import heuristics as Hh
    from s3grl_amd import mpgnn, ncn

    sp = split_of(name)

    def both(r):
        return {k: [round(v[0], 6), round(v[1], 6)] for k, v in r.items()}

    out = {"num_nodes": sp.num_nodes, "epochs": epochs, "CN": both(Hh.run_heuristic(sp, "CN")),
           "run_mpgnn_GCN": both(mpgnn.run_mpgnn(sp, "GCN", epochs=epochs))}
    for use_cn in (True, False):
        for mask in (True, False):
            t0 = time.perf_counter()
            r = both(ncn.run_ncn(sp, epochs=epochs, use_cn=use_cn, mask=mask))
            r["wall_s"] = round(time.perf_counter() - t0, 2)
            out[f"run_ncn_use_cn_{use_cn}_mask_{mask}"] = r
            print(name, use_cn, mask, json.dumps(r), flush=True)
    return out


def usair_test_shape():
    """what tests/test_gpu_ncn.py runs: USAir, 8 epochs, hidden 64"""
    from heuristics_probe import split_of
    from s3grl_amd import ncn

    history = []
    r = ncn.run_ncn(split_of("usair"), epochs=8, hidden=64, seed=1, history=history)
    steps = len(history) // 8
    return {"epochs": 8, "hidden": 64, "first_epoch_loss": round(float(np.mean(history[:steps])), 4),
            "last_epoch_loss": round(float(np.mean(history[-steps:])), 4),
            "AUC": [round(v, 6) for v in r["AUC"]], "AP": [round(v, 6) for v in r["AP"]]}


def kernel_times(trace):
    """Median kernel time per list and phase from a rocprofv3 kernel trace of a --quick run: per list the object is
    built 1 + WARMUP + REPEATS times (a count and a fill launch each), then come WARMUP + REPEATS forward sums,
    as many backward sums, and one more of each."""
    with open(trace, newline="") as f:
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f))
    lists = [e - b for b, e, k in rows if "cn_lists_kernel" in k]
    sums = [e - b for b, e, k in rows if "segment_sum_kernel" in k]
    per = WARMUP + REPEATS
    if len(lists) != 2 * 2 * (per + 1) or len(sums) != 2 * (2 * per + 2):
        raise SystemExit(f"expected {4 * (per + 1)} list and {4 * per + 4} sum dispatches, found {len(lists)}, {len(sums)}")

    def stats(ns):
        return {"median_us": round(float(np.median(ns)) / 1e3, 2), "min_us": round(min(ns) / 1e3, 2),
                "max_us": round(max(ns) / 1e3, 2)}

    out = {}
    for at, name in enumerate(("random", "entries")):
        mine = lists[at * 2 * (per + 1):(at + 1) * 2 * (per + 1)][-2 * REPEATS:]
        fwd_bwd = sums[at * (2 * per + 2):(at + 1) * (2 * per + 2)]
        out[name] = {"count": stats(mine[0::2]), "fill": stats(mine[1::2]),
                     "forward": stats(fwd_bwd[WARMUP:per]), "backward": stats(fwd_bwd[per + WARMUP:2 * per])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "ncn_probe.json"))
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--kernel-trace")
    args = ap.parse_args()
    if args.kernel_trace:
        res = json.loads(Path(args.out).read_text())
        kt = kernel_times(args.kernel_trace)
        res["kernel_source"] = ("a separate process: `rocprofv3 --kernel-trace --stats -- python tools/ncn_probe.py "
                                "--quick`, the same calls in the same order; the wall times under `hip` are from the "
                                "untraced full run")
        for name, row in kt.items():
            model = res["pubmed"]["lists"][name]["modelled_bytes"]
            for k in ("forward", "backward"):
                rate = model[k] / (row[k]["median_us"] * 1e-6)
                row[k]["modelled_TB_per_s"] = round(rate / 1e12, 3)
                row[k]["share_of_random_row_rate"] = round(rate / RANDOM_ROW_RATE, 3)
            res["pubmed"]["lists"][name]["kernel"] = row
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(kt))
        return
    import torch

    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS,
           "times": "host clock around a call that ends in a device synchronise",
           "random_row_rate_B_per_s": RANDOM_ROW_RATE, "random_row_rate_note": RANDOM_ROW_RATE_NOTE}
    res["pubmed"] = pubmed(args.quick)
    if args.quick:
        return
    res["usair_test_shape"] = usair_test_shape()
    res["auc"] = {name: auc_rows(name, args.epochs) for name in ("usair", "cora")}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
