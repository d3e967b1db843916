#!/usr/bin/env python3
"""Generate tests/golden/gic_*.npz — REFERENCE-PINNED Graph InfoClust forward / backward passes.  Run in the BUILD
CONTAINER only (`python tests/golden/make_gic_golden.py`); the reference does not exist on the GPU box.

Executes the reference's own `models.gic.GIC` (Software/GIC), `process.normalize_adj` and, for the fp32 run,
`process.sparse_mx_to_torch_sparse_tensor`, the way GICEmbs.py:CalGIC sets them up, once in fp64 and once in fp32 on
the same inputs.  Parameters, `init` and x are drawn on a 2^-12 grid (exact in fp32, and they compress).  Stored:
    arcs [E, 2] (src, dst), num_nodes, x (or x_is_eye = 1), perm, beta, alpha, K, dim
    p_<name>           every parameter of the reference's state_dict, and init                      (fp64)
    op_row / op_col / op_val   normalize_adj(A + I) as COO, out = M @ h                             (fp64)
    h1 h2 mu10 Z S logits logits2 loss   forward; mu10 = mu after the 10 detached iterations        (fp64)
    g_<name>           the gradient of every parameter                                              (fp64)
    embed_H embed_c    embed()'s S @ Z and c (its h1 and Z are h1 and Z above)                      (fp64)
    f32_<key>          the fp32 run's copy of every output above
An output of more than 16384 elements (case `wide` only) is stored as a fixed subset of its rows, `<key>_rows` naming
them, to keep the file small; the host test pins the restatement to them and the GPU tests compare whole arrays
against the restatement.  Only inputs and expected outputs are stored; no reference source text.
"""
import os
import sys
from pathlib import Path

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import scipy.sparse as sp
import torch

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path.insert(0, str(HERE))

from make_golden import REFERENCE  # noqa: E402
GRID = 4096.0
BIG = 16384

OUTPUTS = ["h1", "h2", "mu10", "Z", "S", "logits", "logits2", "loss", "embed_H", "embed_c"]


def grid(t):
    return torch.round(t * GRID) / GRID


def cases():
    rng = np.random.default_rng(7)
    tiny = np.array([[0, 1], [1, 2], [1, 2], [2, 0], [3, 3], [4, 1], [0, 4]])      # a duplicate, a loop; node 5 isolated
    yield dict(name="tiny", n=6, arcs=tiny, f=3, d=5, K=3, beta=10, alpha=0.75, seed=0)
    a = rng.integers(0, 300, size=(900, 2))
    a = a[a[:, 0] < a[:, 1]]
    yield dict(name="rand300", n=300, arcs=a, f=16, d=32, K=10, beta=100, alpha=0.5, seed=1)
    sys.path.insert(0, str(REPO))
    from s3grl_amd import workloads

    n, e = workloads.load_topology("usair")
    split = workloads.edge_split(n, e, seed=1)
    yield dict(name="usair", n=n, arcs=np.asarray(split.edge_index()).T, f=None, d=32, K=10, beta=100, alpha=0.5,
               seed=2)
    a = rng.integers(0, 200, size=(500, 2))
    a = a[a[:, 0] != a[:, 1]]
    yield dict(name="wide", n=200, arcs=np.concatenate([a, a[:, ::-1]]), f=24, d=256, K=128, beta=100, alpha=0.5,
               seed=3)
    a = rng.integers(0, 130, size=(400, 2))
    yield dict(name="odd", n=130, arcs=np.concatenate([a, a[:40]]), f=11, d=37, K=7, beta=10, alpha=0.75, seed=4)


def run(GIC, process, cluster_fn, case, params, init, x, perm, dtype):
    n, d, K, beta = case["n"], case["d"], case["K"], case["beta"]
    arcs = case["arcs"]
    A = sp.coo_matrix((np.ones(len(arcs)), (arcs[:, 0], arcs[:, 1])), shape=(n, n)).tocsr()   # duplicates add up
    M = process.normalize_adj(A + sp.eye(n))
    if dtype == torch.float32:
        adj = process.sparse_mx_to_torch_sparse_tensor(M)
    else:
        M = M.tocoo()
        adj = torch.sparse_coo_tensor(np.vstack((M.row, M.col)).astype(np.int64), torch.from_numpy(M.data), M.shape)
    M = M.tocoo()
    model = GIC(n, x.shape[1], d, "prelu", K, beta).to(dtype)
    model.load_state_dict({k: v.to(dtype) for k, v in params.items()})
    model.cluster.init = init.to(dtype)
    feats = x.to(dtype)[None]
    shuf = feats[:, perm, :]
    model.train()
    logits, logits2 = model(feats, shuf, adj, True, None, None, None, beta)
    lbl = torch.cat((torch.ones(1, n), torch.zeros(1, n)), 1).to(dtype)
    bce = torch.nn.BCEWithLogitsLoss()
    loss = case["alpha"] * bce(logits, lbl) + (1 - case["alpha"]) * bce(logits2, lbl)
    loss.backward()
    out = {"logits": logits, "logits2": logits2, "loss": loss}
    out.update({"g_" + k: p.grad for k, p in model.named_parameters()})
    with torch.no_grad():
        h1 = model.gcn(feats, adj, True)[0]
        out["h1"], out["h2"] = h1, model.gcn(shuf, adj, True)[0]
        out["mu10"] = cluster_fn(h1, K, 1, 10, init=init.to(dtype), cluster_temp=torch.tensor(beta))[0]
        out["Z"], out["S"] = model.cluster(h1, beta)
        model.eval()
        e_h1, out["embed_H"], out["embed_c"], e_Z = model.embed(feats, adj, True, None, beta)
        assert torch.equal(e_h1[0], h1) and torch.equal(e_Z, out["Z"])
    return {k: v.detach().numpy() for k, v in out.items()}, M


def main():
    for p in ("", "models", "utils"):
        sys.path.insert(0, str(REFERENCE / "Software" / "GIC" / p))
    from gic import GIC          # noqa: E402  (the reference modules)
    import process               # noqa: E402
    from layers.cluster import cluster as cluster_fn   # noqa: E402

    for case in cases():
        n, d, K = case["n"], case["d"], case["K"]
        torch.manual_seed(case["seed"])
        f = n if case["f"] is None else case["f"]
        x = torch.eye(n) if case["f"] is None else grid(torch.randn(n, f))
        proto = GIC(n, f, d, "prelu", K, case["beta"])
        params = {k: grid(v.detach()) for k, v in proto.state_dict().items()}
        params["gcn.bias"] = grid(0.1 * torch.randn(d))            # off their zero init, so every path carries signal
        params["disc.f_k.bias"] = grid(0.1 * torch.randn(1))
        init = grid(torch.rand(K, d))
        perm = torch.randperm(n)
        o64, M = run(GIC, process, cluster_fn, case, params, init, x, perm, torch.float64)
        o32, _ = run(GIC, process, cluster_fn, case, params, init, x, perm, torch.float32)
        blob = {"arcs": case["arcs"].astype(np.int64), "num_nodes": np.int64(n), "perm": perm.numpy(),
                "beta": np.float64(case["beta"]), "alpha": np.float64(case["alpha"]), "K": np.int64(K),
                "dim": np.int64(d), "x_is_eye": np.int64(case["f"] is None),
                "op_row": M.row.astype(np.int64), "op_col": M.col.astype(np.int64), "op_val": M.data.astype(np.float64)}
        if case["f"] is not None:
            blob["x"] = x.double().numpy()
        for k, v in params.items():
            blob["p_" + k] = v.double().numpy()
        blob["p_init"] = init.double().numpy()
        for k, v in o64.items():
            assert np.isfinite(v).all() and np.isfinite(o32[k]).all(), (case["name"], k)
            v64, v32 = np.asarray(v, dtype=np.float64), np.asarray(o32[k], dtype=np.float32)
            if v64.size > BIG:
                v64, v32 = v64.reshape(-1, v64.shape[-1]), v32.reshape(-1, v32.shape[-1])
                rows = np.arange(0, v64.shape[0], -(-v64.shape[0] // max(1, 4096 // v64.shape[1])))
                blob[k + "_rows"] = rows
                v64, v32 = v64[rows], v32[rows]
            blob[k], blob["f32_" + k] = v64, v32
        out = HERE / f"gic_{case['name']}.npz"
        np.savez_compressed(out, **blob)
        print(f"{out.name}: N={n} E={len(case['arcs'])} d={d} K={K}  {out.stat().st_size} bytes  "
              f"logits2 fp32-vs-fp64 {np.abs(o32['logits2'] - o64['logits2']).max():.2e}")


if __name__ == "__main__":
    if not REFERENCE.exists():
        sys.exit("needs the reference checkout (build container only)")
    main()
