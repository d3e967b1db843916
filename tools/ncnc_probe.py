"""NCNC probe -> profiles/ncnc_probe.json.

PubMed (seed-0 train graph), H = 256, the 164 000 stored entries of the train graph taken cyclically as links, with
exclude_endpoints on.  WARMUP calls and then REPEATS timed ones, medians reported, every timed call ending in a device
synchronise, of
  build       `SplitNeighbours` from the device CSR and device links (count, scan, fill, the host's id checks)
  transpose   the stable sort behind `.t_ptr` / `.t_link` / `.t_perm`
  forward     `s3grl_segment_wsum` over the lists (what `completed_neighbour_sum` runs)
  backward_z  `s3grl_segment_wsum` over the transposed lists, with the gather of the weights into transposed order
  backward_w  `s3grl_segment_dot`
against (a) the same steps in plain torch on the same GPU: `index_select` of the rows, a multiply, and `index_add_`
into the output (forward, backward_z) or a row sum (backward_w); the split build has no plain-torch comparator here
and is listed as not measured; and (b) the numpy restatement (tests/ncnc_reference.py) on this machine's CPUs, on the
first CPU_LINKS links only (it is a Python loop), beside the HIP calls on the same prefix, with a check that the HIP
outputs equal it to the bit.
USAir and Cora (seed-0 splits, no node features): test AUC / AP of `run_ncnc` beside `run_ncn` and CN.

    python tools/ncnc_probe.py [--out profiles/ncnc_probe.json] [--epochs 50] [--quick]

`--quick` skips the CPU restatement and the AUC rows and writes nothing.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
sys.path.insert(0, str(REPO / "tools"))

from ncn_probe import H, MANY, REPEATS, WARMUP, gpu_times, link_lists  # noqa: E402

CPU_LINKS = 20000


def torch_steps(z, g, w, owner, idx, L, n):
    """the three products in plain torch: gather, multiply, index_add_ / row sum"""
    import torch

    def forward():
        return torch.zeros((L, z.shape[1]), device=z.device).index_add_(0, owner, z.index_select(0, idx) * w[:, None])

    def backward_z():
        return torch.zeros((n, z.shape[1]), device=z.device).index_add_(0, idx, g.index_select(0, owner) * w[:, None])

    def backward_w():
        return (g.index_select(0, owner) * z.index_select(0, idx)).sum(1)

    return {"forward": forward, "backward_z": backward_z, "backward_w": backward_w}


def bits_equal(t, ref):
    a = t.cpu().numpy()
    return a.shape == ref.shape and a.dtype == ref.dtype and bool(np.array_equal(a.view(np.uint8), ref.view(np.uint8)))


def pubmed(quick):
    import torch

    import ncnc_reference as R
    from heuristics_probe import split_of
    from s3grl_amd import ncn
    from s3grl_amd.heuristics import canonical_csr

    sp = split_of("pubmed")
    A = canonical_csr(sp.A)
    n, deg = sp.num_nodes, np.diff(A.indptr)
    g0 = ncn._TrainGraph(A)
    dev = g0.engine.device
    links = link_lists(sp)["entries"]
    l_d = torch.as_tensor(links).to(dev)
    z_np, g_np = R.values((n, H), seed=1), R.values((MANY, H), seed=2)
    z, g = torch.as_tensor(z_np).to(dev), torch.as_tensor(g_np).to(dev)
    sn = ncn.SplitNeighbours(g0.csr(), l_d, True)
    total = int(sn.idx.numel())
    w_np = R.weights(total, seed=3)
    w = torch.as_tensor(w_np).to(dev)
    counts = sn.counts.sum(1).tolist()
    out = {"num_nodes": n, "nnz": int(A.nnz), "H": H, "links": MANY, "exclude_endpoints": True, "entries": total,
           "section_entries": counts, "mean_entries_per_link": round(total / MANY, 3),
           "longest_list": int(sn.ptr.diff().max()), "max_links_per_node": int(sn.t_ptr.diff().max()),
           "inner_pairs": int(sn.inner_at.numel()),
           "mean_endpoint_degree": round(float(deg[links].mean()), 2)}
    key_bytes = int(4 * (deg[links[0]].sum() + deg[links[1]].sum()))
    out["modelled_bytes"] = {"build": 4 * key_bytes + 2 * 8 * total, "forward": total * (H * 4 + 8) + MANY * H * 4,
                             "backward_z": total * (H * 4 + 8) + n * H * 4, "backward_w": total * (H * 4 + 8) + MANY * H * 4,
                             "note": "build: both rows' keys walked once and searched once, in count and in fill, plus "
                                     "idx and side written; sums: entries·H·4 gathered, id and weight per entry, the "
                                     "output written; dot: entries·H·4 gathered, the g rows, ids read and out_w written"}

    def transpose():
        sn._t = None
        sn.t_link

    hip = {"build": gpu_times(lambda: ncn.SplitNeighbours(g0.csr(), l_d, True)),
           "transpose": gpu_times(transpose),
           "forward": gpu_times(lambda: ncn._segment_wsum(z, sn.ptr, sn.idx, w, MANY)),
           "backward_z": gpu_times(lambda: ncn._segment_wsum(g, sn.t_ptr, sn.t_link, w[sn.t_perm].contiguous(), n)),
           "backward_w": gpu_times(lambda: ncn._segment_dot(g, z, sn.ptr, sn.idx))}
    for k in ("build", "forward", "backward_z", "backward_w"):
        hip[k]["modelled_TB_per_s_wall"] = round(out["modelled_bytes"][k] / hip[k]["median_s"] / 1e12, 4)
    out["hip"] = hip
    print("hip", json.dumps(hip), flush=True)
    owner = torch.repeat_interleave(torch.arange(MANY, device=dev), sn.ptr.diff(), output_size=total)
    steps = torch_steps(z, g, w, owner, sn.idx.long(), MANY, n)
    try:
        out["torch_same_gpu"] = {k: gpu_times(fn) for k, fn in steps.items()}
        out["torch_same_gpu"]["build"] = {"not_measured": "no plain-torch comparator for the three-way row split"}
        mine = {"forward": ncn._segment_wsum(z, sn.ptr, sn.idx, w, MANY),
                "backward_z": ncn._segment_wsum(g, sn.t_ptr, sn.t_link, w[sn.t_perm].contiguous(), n),
                "backward_w": ncn._segment_dot(g, z, sn.ptr, sn.idx)}
        out["torch_max_abs_difference"] = {k: float((steps[k]() - mine[k]).abs().max()) for k in steps}
        out["hip_speedup_over_torch"] = {k: round(out["torch_same_gpu"][k]["median_s"] / hip[k]["median_s"], 2)
                                         for k in steps}
    except Exception as e:          # an operator this torch build lacks, or memory: said, not hidden
        out["torch_same_gpu"] = {"not_measured": f"{type(e).__name__}: {e}"[:300]}
    print("torch", json.dumps(out["torch_same_gpu"]), flush=True)
    if quick:
        return out
    few = links[:, :CPU_LINKS]
    f_d = l_d[:, :CPU_LINKS].contiguous()
    small = ncn.SplitNeighbours(g0.csr(), f_d, True)
    t = [time.perf_counter()]
    cnt, ptr, idx, side = R.split_lists(A, few, True)
    t.append(time.perf_counter())
    ws, gs = w_np[:len(idx)], g_np[:CPU_LINKS]
    ref_f = R.segment_wsum(z_np, ptr, idx, ws)
    t.append(time.perf_counter())
    ref_z = R.wsum_grad_z(gs, ptr, idx, ws, n)
    t.append(time.perf_counter())
    ref_w = R.segment_dot(gs, z_np, ptr, idx)
    t.append(time.perf_counter())
    cpu = dict(zip(("build", "forward", "backward_z", "backward_w"), (round(b - a, 4) for a, b in zip(t, t[1:]))))
    w_s, g_s = w[:len(idx)].contiguous(), g[:CPU_LINKS].contiguous()
    hip_few = {"build": gpu_times(lambda: ncn.SplitNeighbours(g0.csr(), f_d, True)),
               "forward": gpu_times(lambda: ncn._segment_wsum(z, small.ptr, small.idx, w_s, CPU_LINKS)),
               "backward_z": gpu_times(lambda: ncn._segment_wsum(g_s, small.t_ptr, small.t_link,
                                                                 w_s[small.t_perm].contiguous(), n)),
               "backward_w": gpu_times(lambda: ncn._segment_dot(g_s, z, small.ptr, small.idx))}
    at, pairs = R.inner_pairs(few, ptr, idx, side)
    same = {"counts": bits_equal(small.counts, cnt), "ptr": bits_equal(small.ptr, ptr), "idx": bits_equal(small.idx, idx),
            "side": bits_equal(small.side, side), "inner_at": bits_equal(small.inner_at, at),
            "inner_links": bits_equal(small.inner_links, pairs),
            "forward": bits_equal(ncn._segment_wsum(z, small.ptr, small.idx, w_s, CPU_LINKS), ref_f),
            "backward_z": bits_equal(ncn._segment_wsum(g_s, small.t_ptr, small.t_link, w_s[small.t_perm].contiguous(), n),
                                     ref_z),
            "backward_w": bits_equal(ncn._segment_dot(g_s, z, small.ptr, small.idx), ref_w)}
    out["prefix"] = {"links": CPU_LINKS, "entries": int(len(idx)), "numpy_cpu_s": cpu, "hip": hip_few,
                     "hip_speedup_over_numpy": {k: round(cpu[k] / hip_few[k]["median_s"], 1) for k in cpu},
                     "hip_bit_equal_to_numpy": same}
    print("numpy", json.dumps(cpu), "bit equal", json.dumps(same), flush=True)
    return out


def auc_rows(name, epochs):
    from heuristics_probe import split_of
    from s3grl_amd import heuristics as Hh
    from s3grl_amd import ncn

    sp = split_of(name)

    def both(r):
        return {k: [round(v[0], 6), round(v[1], 6)] for k, v in r.items()}

    out = {"num_nodes": sp.num_nodes, "epochs": epochs, "CN": both(Hh.run_heuristic(sp, "CN"))}
    for what, fn in (("run_ncn", ncn.run_ncn), ("run_ncnc", ncn.run_ncnc)):
        t0 = time.perf_counter()
        r = both(fn(sp, epochs=epochs))
        r["wall_s"] = round(time.perf_counter() - t0, 2)
        out[what] = r
        print(name, what, json.dumps(r), flush=True)
    return out


def usair_test_shape():
    """what tests/test_gpu_ncnc.py runs: USAir, 8 epochs, hidden 64"""
    from heuristics_probe import split_of
    from s3grl_amd import ncn

    out = {"epochs": 8, "hidden": 64}
    for what, fn in (("run_ncnc", ncn.run_ncnc), ("run_ncn", ncn.run_ncn)):
        history = []
        t0 = time.perf_counter()
        r = fn(split_of("usair"), epochs=8, hidden=64, seed=1, history=history)
        steps = len(history) // 8
        out[what] = {"first_epoch_loss": round(float(np.mean(history[:steps])), 4),
                     "last_epoch_loss": round(float(np.mean(history[-steps:])), 4),
                     "AUC": [round(v, 6) for v in r["AUC"]], "AP": [round(v, 6) for v in r["AP"]],
                     "wall_s": round(time.perf_counter() - t0, 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "ncnc_probe.json"))
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    import torch

    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS,
           "times": "host clock around a call that ends in a device synchronise"}
    res["pubmed"] = pubmed(args.quick)
    if args.quick:
        return
    res["usair_test_shape"] = usair_test_shape()
    print("usair test shape", json.dumps(res["usair_test_shape"]), flush=True)
    res["auc"] = {name: auc_rows(name, args.epochs) for name in ("usair", "cora")}
    res["not_measured"] = ["any hardware counter or kernel-only time (all figures are host wall times)",
                           "a plain-torch split build", "the CPU restatement beyond the first CPU_LINKS links",
                           "H other than 256", "more than one seed of run_ncnc", "node features",
                           "a graph with rows of tens of thousands of keys"]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
