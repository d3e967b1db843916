#!/usr/bin/env python3
"""Generate tests/golden/labels_*.npz — REFERENCE-PINNED labelled enclosing subgraphs.  Run in the BUILD
CONTAINER only (`python tests/golden/make_label_golden.py`); the reference does not exist on the GPU box.

For the links of the extraction fixtures (extract_*.npz, extract_directed_*.npz: same graphs, same links,
same hops) this executes the reference's own `utils.k_hop_subgraph` followed by `utils.construct_pyg_graph`
(reference utils.py:47-85, :277-316) for every node label, importing the reference the way make_golden.py
does.  `Data` there is swapped for an inert attribute holder.  Stored per case and hop, ragged arrays
concatenated with offsets (one entry per link):
    h{h}_nodes         node ids: src, dst, then hop-major and ascending id inside a hop (the engine's order;
                       the reference's is CPython set order there)
    h{h}_z_{label}     z of those nodes, in the same order ([n] or [n, 2])
    h{h}_edges         (global u, global v, weight) of ssp.find's triples, sorted
Labels: drnl, de, de+, hop, zo, degree and "none" (any other name: zeros).
Only inputs and expected outputs are stored; no reference source text.
"""
import os
import sys
from pathlib import Path

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True

import numpy as np
import scipy.sparse as ssp

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import make_golden  # noqa: E402

LABELS = ["drnl", "de", "de+", "hop", "zo", "degree", "none"]
CASES = [("triangle", False), ("pair", False), ("star_iso", False), ("probe5", False), ("rand300", False),
         ("usair", False), ("cora", False), ("tiny", True), ("usair", True)]


class Holder:
    """Inert stand-in for torch_geometric.data.Data: keeps what it is given."""

    def __init__(self, x=None, edge_index=None, **kw):
        self.x = x
        self.edge_index = edge_index
        self.__dict__.update(kw)


def tag(label):
    return {"de+": "deplus"}.get(label, label)


def main():
    ref = make_golden.import_reference_utils()
    ref.Data = Holder
    for name, directed in CASES:
        src = np.load(HERE / (f"extract_directed_{name}.npz" if directed else f"extract_{name}.npz"))
        n = int(src["num_nodes"])
        if directed:
            arcs = src["arcs"].astype(np.int64)
            A = ssp.csr_matrix((np.ones(len(arcs), dtype=np.int64), (arcs[:, 0], arcs[:, 1])), shape=(n, n))
            A_csc = A.tocsc()
        else:
            A = make_golden.csr_from_undirected(n, src["edges"])
            A_csc = None
        links = src["links"].astype(np.int64)
        hops = [int(h) for h in src["hops"]]
        blob = {"num_nodes": np.int64(n), "links": links, "hops": np.asarray(hops), "directed": np.int64(directed)}
        blob["arcs" if directed else "edges"] = src["arcs" if directed else "edges"]
        for h in hops:
            cat = {"nodes": [], "edges": []}
            cat.update({f"z_{tag(lb)}": [] for lb in LABELS})
            for s, d in links:
                nodes, sub, dists, _, y = ref.k_hop_subgraph(int(s), int(d), h, A, 1.0, None, node_features=None,
                                                             y=1, directed=directed, A_csc=A_csc)
                rest = np.lexsort((np.asarray(nodes[2:]), np.asarray(dists[2:])))
                order = np.concatenate([[0, 1], 2 + rest]).astype(np.int64)   # src, dst first
                gid = np.asarray(nodes, dtype=np.int64)
                cat["nodes"].append(gid[order].astype(np.int32))
                for lb in LABELS:
                    data = ref.construct_pyg_graph(nodes, sub.copy(), dists, None, y, lb)
                    z = data.z.numpy().astype(np.int32)
                    cat[f"z_{tag(lb)}"].append(z[order])
                    if lb == "drnl":
                        ei = data.edge_index.numpy()
                        w = np.asarray(data.edge_weight).astype(np.int64)
                        trip = np.stack([gid[ei[0]], gid[ei[1]], w], axis=1)
                        cat["edges"].append(trip[np.lexsort((trip[:, 1], trip[:, 0]))].astype(np.int32))
            for k, parts in cat.items():
                off = np.zeros(len(parts) + 1, dtype=np.int64)
                np.cumsum([len(p) for p in parts], out=off[1:])
                blob[f"h{h}_{k}"] = np.concatenate(parts, axis=0)
                blob[f"h{h}_{k}_off"] = off
        out = f"labels_directed_{name}.npz" if directed else f"labels_{name}.npz"
        np.savez_compressed(HERE / out, **blob)
        print(f"{out}: {len(links)} links x hops {hops} x {len(LABELS)} labels")


if __name__ == "__main__":
    if not make_golden.REFERENCE.exists():
        sys.exit("needs the reference checkout (build container only)")
    main()
