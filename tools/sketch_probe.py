"""Subgraph-sketch probe -> profiles/sketch_probe.json.

PubMed (seed-0 train split, hops 2, num_perm 128, hll_p 8):
  * wall time of `SketchGraph(A)` (upload, host check, init and one propagate launch per hop, ending in a device
    synchronise) and of `features(links)` on the split's val / test links and on 164 000 random pairs (host id check,
    upload, the pairs kernel, a device synchronise): WARMUP calls, then REPEATS timed ones; median, min and max;
  * the same work (a) by the numpy restatement (tests/sketch_reference.py) on this machine's CPUs and (b) on the
    same GPU in plain torch: propagation by `scatter_reduce(amin / amax)` over the gathered neighbour rows, the pair
    step by row compares, a register look-up table and torch arithmetic; both are checked against the HIP outputs;
USAir and Cora (seed-0 splits, no node features): test AUC of `run_buddy`, of `run_heuristic(split, "CN")`, and of
the same `BuddyTwin` trained on the exact counts (`sketch_reference.exact_counts`) in place of the sketch estimates.

    python tools/sketch_probe.py [--out profiles/sketch_probe.json] [--epochs 50] [--quick]

`--quick` runs only the HIP timings (for a kernel trace of its own).
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

import sketch_reference as R  # noqa: E402
from heuristics_probe import split_of  # noqa: E402
from s3grl_amd import heuristics as H  # noqa: E402
from s3grl_amd import sketch as S  # noqa: E402

HOPS, P, HLL_P = 2, 128, 8
WARMUP, REPEATS = 3, 20


def gpu_times(fn, warmup=WARMUP, repeats=REPEATS):
    """wall seconds of fn() + device synchronise: {'median', 'min', 'max', 'repeats'}"""
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


def cpu_time(fn, repeats=2):
    ts, out = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, round(min(ts), 4)


class TorchSketch:
    """The same sketches and features in plain torch on the device (the baseline, not a product path)."""

    def __init__(self, A, hops, num_perm, hll_p, seed, device):
        A = H.canonical_csr(A)
        self.hops, self.P, self.p, self.dev = hops, num_perm, hll_p, device
        n = A.shape[0]
        self.row = torch.as_tensor(np.repeat(np.arange(n), np.diff(A.indptr)).astype(np.int64)).to(device)
        self.col = torch.as_tensor(A.indices.astype(np.int64)).to(device)
        h = R.hashes(np.arange(n), num_perm + 1, seed)                       # hop 0 from the host, not timed apart
        self.mh0 = torch.as_tensor((h[:, :num_perm] ^ np.uint32(1 << 31)).view(np.int32)).to(device)   # order-preserving
        hl0 = np.zeros((n, 1 << hll_p), dtype=np.uint8)
        hh = h[:, num_perm]
        hl0[np.arange(n), hh >> np.uint32(32 - hll_p)] = R.rank(hh & np.uint32((1 << (32 - hll_p)) - 1), hll_p)
        self.hl0 = torch.as_tensor(hl0).to(device)
        m, C, lc = S.hll_constants(hll_p)
        self.m, self.C, self.lc = m, C, torch.as_tensor(lc).to(device)
        self.pow2 = torch.as_tensor((2 ** np.clip(33 - hll_p - np.arange(256), 0, None)).astype(np.int64)).to(device)
        self.hl_dtype = torch.uint8

    def propagate(self):
        mh, hl = [self.mh0], [self.hl0.to(self.hl_dtype)]
        for _ in range(self.hops):
            a = mh[-1].clone()
            a.scatter_reduce_(0, self.row[:, None].expand(-1, a.shape[1]), mh[-1][self.col], "amin", include_self=True)
            b = hl[-1].clone()
            b.scatter_reduce_(0, self.row[:, None].expand(-1, b.shape[1]), hl[-1][self.col], "amax", include_self=True)
            mh.append(a)
            hl.append(b)
        self.mh, self.hl = torch.stack(mh), torch.stack(hl)
        return self.mh, self.hl

    def card(self, regs):
        T = self.pow2[regs.long()].sum(-1)
        z = (regs == 0).sum(-1)
        raw = self.C / T.double()
        return torch.where((raw <= 2.5 * self.m) & (z > 0), self.lc[z], raw)

    def features(self, links):
        u, v = links
        K = self.hops + 1
        zero = torch.zeros(links.shape[1], dtype=torch.float64, device=self.dev)
        I = [[((self.mh[i][u] == self.mh[j][v]).sum(1).double() * self.card(torch.maximum(self.hl[i][u], self.hl[j][v])))
              / float(self.P) for j in range(K)] for i in range(K)]
        Eu, Ev = [self.card(self.hl[i][u]) for i in range(K)], [self.card(self.hl[i][v]) for i in range(K)]

        def at(i, j):
            return zero if i < 0 or j < 0 else I[i][j]

        def A(i, j):
            return ((at(i, j) - at(i - 1, j)) - at(i, j - 1)) + at(i - 1, j - 1)

        cols = [A(i, j) for i in range(1, K) for j in range(1, K)]
        for side, E in ((0, Eu), (1, Ev)):
            for i in range(1, K):
                s = zero
                for j in range(K):
                    s = s + (A(j, i) if side else A(i, j))
                cols.append((E[i] - E[i - 1]) - s)
        return torch.stack(cols, dim=1).float()


def pubmed(quick):
    sp = split_of("pubmed")
    A = sp.A
    val_test = np.concatenate([sp.links["valid"][0], sp.links["valid"][1], sp.links["test"][0], sp.links["test"][1]],
                              axis=1)
    many = np.random.default_rng(0).integers(0, sp.num_nodes, size=(2, 164000)).astype(np.int64)
    out = {"num_nodes": sp.num_nodes, "nnz": int(A.nnz), "hops": HOPS, "num_perm": P, "hll_p": HLL_P,
           "val_test_links": int(val_test.shape[1]), "many_links": int(many.shape[1]),
           "table_bytes_per_hop": int(sp.num_nodes * (4 * P + (1 << HLL_P)))}
    out["hip"] = {"build": gpu_times(lambda: S.SketchGraph(A, HOPS, P, HLL_P).close())}
    sk = S.SketchGraph(A, HOPS, P, HLL_P)
    out["hip"]["features_val_test"] = gpu_times(lambda: sk.features(val_test))
    out["hip"]["features_many"] = gpu_times(lambda: sk.features(many))
    out["hip"]["ball_sizes"] = gpu_times(sk.ball_sizes)
    if quick:
        sk.close()
        return out
    dev = sk.engine.device
    # (a) the numpy restatement on the CPUs
    (mh, hl), t = cpu_time(lambda: R.sketches(A, HOPS, P, HLL_P, 0))
    out["numpy"] = {"build_s": t, "threads": torch.get_num_threads()}
    ref_vt, out["numpy"]["features_val_test_s"] = cpu_time(lambda: R.link_outputs(mh, hl, val_test, HLL_P), 1)
    ref_many, out["numpy"]["features_many_s"] = cpu_time(lambda: R.link_outputs(mh, hl, many, HLL_P), 1)
    out["hip"]["bit_equal_to_numpy"] = bool(
        np.array_equal(sk.minhash.cpu().numpy().view(np.uint32), mh) and np.array_equal(sk.hll.cpu().numpy(), hl)
        and np.array_equal(sk.features(val_test).cpu().numpy().view(np.uint32), ref_vt["features"].view(np.uint32))
        and np.array_equal(sk.features(many).cpu().numpy().view(np.uint32), ref_many["features"].view(np.uint32)))
    # (b) plain torch on the same GPU
    ts = TorchSketch(A, HOPS, P, HLL_P, 0, dev)
    try:
        ts.propagate()
    except RuntimeError as e:                        # scatter_reduce without a uint8 kernel: registers as int32
        ts.hl_dtype = torch.int32
        out["torch_note"] = f"uint8 scatter_reduce refused ({str(e)[:80]}); HLL registers held as int32"
        ts.propagate()
    out["torch"] = {"build": gpu_times(ts.propagate)}
    vt_d, many_d = torch.as_tensor(val_test).to(dev), torch.as_tensor(many).to(dev)
    out["torch"]["features_val_test"] = gpu_times(lambda: ts.features(vt_d))
    out["torch"]["features_many"] = gpu_times(lambda: ts.features(many_d), warmup=2, repeats=5)
    out["torch"]["equal_to_hip"] = bool(
        torch.equal((ts.mh ^ (-2 ** 31)).int(), sk.minhash) and torch.equal(ts.hl.to(torch.uint8), sk.hll)
        and torch.equal(ts.features(vt_d), sk.features(val_test)))
    sk.close()
    for kind in ("build", "features_val_test", "features_many"):
        hip = out["hip"][kind]["median_s"]
        out[f"{kind}_speedup"] = {"vs_numpy": round(out["numpy"][f"{kind}_s"] / hip, 1),
                                  "vs_torch": round(out["torch"][kind]["median_s"] / hip, 2)}
    return out


def auc_rows(name, epochs):
    sp = split_of(name)
    kw = dict(hops=HOPS, epochs=epochs, lr=0.01, seed=1)
    buddy = S.run_buddy(sp, **kw)
    exact = S.run_buddy(sp, structure=lambda links: R.exact_counts(sp.A, links, HOPS)["features"], **kw)
    cn = H.run_heuristic(sp, "CN")

    def both(r):
        return {k: [round(v[0], 6), round(v[1], 6)] for k, v in r.items()}

    return {"num_nodes": sp.num_nodes, "epochs": epochs, "run_buddy": both(buddy),
            "buddy_twin_on_exact_counts": both(exact), "CN": both(cn)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "sketch_probe.json"))
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "repeats": REPEATS}
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
