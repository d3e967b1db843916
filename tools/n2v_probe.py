"""node2vec pretraining probe -> profiles/n2v_probe.json.

  * wall time of the paper's 50-epoch pretraining (dim 16, walk 20, context 10, 10 walks, 1 negative, batch 32,
    SparseAdam lr 0.01) on the engine, USAir (train split) and Router (tests/golden/router_edges.txt, all edges),
    host clock around fit() ending in its device read-back; a warm-up fit first;
  * the same on a CPU restatement with the reference's structure: nn.Embedding(sparse=True), SparseAdam, PyG's
    loss, walks drawn in numpy, torch on the CPU threads this process is given (--cpu-epochs epochs, scaled to 50);
  * the three-seed AUCs behind the thresholds of tests/test_gpu_node2vec.py (dot-product AUC on USAir's test
    links, node2vec seeds 0, 1, 2; usair_posplus_k3_n2v end to end, its node2vec seed 0, training seeds 1, 2, 3).

    python tools/n2v_probe.py [--out profiles/n2v_probe.json] [--cpu-epochs 3] [--skip-auc] [--only-engine]

--only-engine runs just the engine's 50-epoch fits (what a `rocprofv3 --kernel-trace --stats` run wraps).
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

from s3grl_amd import workloads as W  # noqa: E402


def graphs():
    n, e = W.load_topology("usair")
    sp = W.edge_split(n, e, seed=0)
    out = {"usair_train": (sp.edge_index(), n)}
    n_r, e_r = W.read_seal_edges(REPO / "tests" / "golden" / "router_edges.txt")
    e_r = W.undirected_unique(e_r)
    out["router_all"] = (np.concatenate([e_r.T, e_r[:, ::-1].T], axis=1), n_r)
    return out


def engine_fit(ei, n, seed=0, epochs=50):
    from s3grl_amd.node2vec import Node2Vec

    n2v = Node2Vec(ei, n, 16, seed=seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    losses = n2v.fit(epochs)      # ends in the read-back of the step losses
    dt = time.perf_counter() - t0
    n2v.close()
    return dt, losses


class CpuNode2Vec:
    """The reference's structure on the CPU: PyG's pos_sample / neg_sample with numpy walks, Node2Vec.loss on
    nn.Embedding(sparse=True), torch.optim.SparseAdam."""

    def __init__(self, ei, n, dim=16, seed=0):
        order = np.argsort(ei[0], kind="stable")
        self.ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.bincount(ei[0], minlength=n), out=self.ptr[1:])
        self.col = ei[1][order]
        self.n = n
        torch.manual_seed(seed)
        self.rng = np.random.default_rng(seed)
        self.emb = torch.nn.Embedding(n, dim, sparse=True)
        self.opt = torch.optim.SparseAdam(list(self.emb.parameters()), lr=0.01)

    def walks(self, batch, L=20):
        rw = [batch]
        cur = batch
        for _ in range(L):
            deg = self.ptr[cur + 1] - self.ptr[cur]
            pick = self.ptr[cur] + (self.rng.random(len(cur)) * np.maximum(deg, 1)).astype(np.int64)
            cur = np.where(deg > 0, self.col[np.minimum(pick, len(self.col) - 1)], cur)
            rw.append(cur)
        return np.stack(rw, 1)

    @staticmethod
    def windows(rw, C=10):
        return torch.as_tensor(np.concatenate([rw[:, j:j + C] for j in range(rw.shape[1] + 1 - C)], 0))

    def loss(self, pos, neg):
        total = 0
        for rw, sign in ((pos, 1), (neg, -1)):
            start, rest = rw[:, 0], rw[:, 1:].contiguous()
            hs = self.emb(start).view(rw.size(0), 1, -1)
            hr = self.emb(rest.view(-1)).view(rw.size(0), -1, hs.shape[-1])
            s = torch.sigmoid((hs * hr).sum(dim=-1).view(-1))
            total = total + (-torch.log((s if sign > 0 else 1 - s) + 1e-15).mean())
        return total

    def epoch(self):
        perm = torch.randperm(self.n).numpy()
        tot = 0.0
        for b in range(0, self.n, 32):
            batch = np.tile(perm[b:b + 32], 10)
            pos = self.windows(self.walks(batch))
            neg_rw = np.concatenate([batch[:, None], self.rng.integers(0, self.n, (len(batch), 20))], 1)
            neg = self.windows(neg_rw)
            self.opt.zero_grad()
            loss = self.loss(pos, neg)
            loss.backward()
            self.opt.step()
            tot += loss.item()
        return tot


def cpu_fit(ei, n, epochs):
    m = CpuNode2Vec(ei, n)
    t0 = time.perf_counter()
    losses = [m.epoch() for _ in range(epochs)]
    return time.perf_counter() - t0, losses


def dot_auc(seed):
    sys.path.insert(0, str(REPO / "tests"))
    from test_gpu_node2vec import _dot_auc

    return _dot_auc(seed)


def e2e_auc(n2v_seed, train_seed):
    from s3grl_amd.engine import Engine
    from s3grl_amd.harness import train_and_evaluate

    n, e = W.load_topology("usair")
    sp = W.edge_split(n, e, seed=0)
    X = W.init_n2v_features(sp, 16, seed=n2v_seed, epochs=50)
    eng = Engine("cuda:0")
    G, f = eng.graph(sp.A), eng.features(X)

    def prep(split):
        pos, neg = sp.links[split]
        li = np.concatenate([pos, neg], axis=1)
        y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
        res = eng.precompute(G, f, eng.links(li), mode="pos_plus", num_hops=2, sign_k=3)
        return res.rows, res.row_ptr, y

    auc, _ = train_and_evaluate(prep("train"), prep("test"), k_heuristic=1, k_pool_strategy="mean", epochs=8,
                                lr=2e-3, seed=train_seed)
    eng.close()
    return auc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(REPO / "profiles" / "n2v_probe.json"))
    ap.add_argument("--cpu-epochs", type=int, default=3)
    ap.add_argument("--skip-auc", action="store_true")
    ap.add_argument("--only-engine", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the MI355X"
    import __graft_entry__ as ge

    ge.build()
    gs = graphs()
    res = {"config": {"dim": 16, "walk_length": 20, "context_size": 10, "walks_per_node": 10,
                      "num_negative_samples": 1, "batch_size": 32, "lr": 0.01, "epochs": 50},
           "graphs": {k: {"num_nodes": int(n), "entries": int(ei.shape[1]), "steps_per_epoch": -(-int(n) // 32)}
                      for k, (ei, n) in gs.items()}}
    engine_fit(*gs["usair_train"], epochs=1)               # warm-up: code objects, allocations
    for k, (ei, n) in gs.items():
        times = [engine_fit(ei, n, seed=s)[0] for s in (0, 1, 2)]
        r = res["graphs"][k]
        r["engine_50_epochs_s"] = times
        r["engine_us_per_step"] = 1e6 * min(times) / (50 * r["steps_per_epoch"])
        print(k, "engine 50 epochs:", [round(t, 3) for t in times], flush=True)
    if not a.only_engine:
        res["cpu_threads"] = torch.get_num_threads()
        for k, (ei, n) in gs.items():
            dt, losses = cpu_fit(ei, n, a.cpu_epochs)
            r = res["graphs"][k]
            r["cpu_epochs_timed"] = a.cpu_epochs
            r["cpu_s_per_epoch"] = dt / a.cpu_epochs
            r["cpu_50_epochs_s_scaled"] = 50 * dt / a.cpu_epochs
            r["cpu_epoch_losses"] = losses
            _, el = engine_fit(ei, n, seed=0, epochs=a.cpu_epochs)
            r["engine_epoch_losses"] = el
            print(k, "cpu s/epoch:", round(dt / a.cpu_epochs, 3), flush=True)
    if not a.skip_auc and not a.only_engine:
        res["dot_auc_usair_seeds_0_1_2"] = [dot_auc(s) for s in (0, 1, 2)]
        print("dot AUC", res["dot_auc_usair_seeds_0_1_2"], flush=True)
        res["e2e_auc_usair_posplus_k3_n2v_seeds_1_2_3"] = [e2e_auc(0, s) for s in (1, 2, 3)]
        print("e2e AUC", res["e2e_auc_usair_posplus_k3_n2v_seeds_1_2_3"], flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1))
    print(json.dumps(res)[:2000])


if __name__ == "__main__":
    main()
