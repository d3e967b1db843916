"""Test infrastructure: a numpy / scipy restatement of the labelled enclosing subgraph of one link
(reference utils.py:211-316, construct_pyg_graph after k_hop_subgraph) for ANY node list — the fixtures'
lists, a sampled plan's, a synthetic star's.  It checks the engine; the product never imports it.

    edges, z = label_subgraph(A, nodes, dists, "drnl")

nodes: global ids, src and dst first.  edges: (local u, local v, weight) int64 [e, 3], sorted — the non-zero
entries of A[nodes][:, nodes] without the target link.  z: int64 [n] or [n, 2].
"""
import numpy as np
import scipy.sparse as ssp
from scipy.sparse.csgraph import shortest_path

LABELS = ["drnl", "de", "de+", "hop", "zo", "degree", "none"]


def induced(A, nodes):
    """A[nodes][:, nodes] with the target link's two entries removed, as COO triples (structure: non-zeros)."""
    nodes = np.asarray(nodes, dtype=np.int64)
    sub = ssp.csr_matrix(A)[nodes][:, nodes].tocoo()
    keep = (sub.data != 0) & ~(((sub.row == 0) & (sub.col == 1)) | ((sub.row == 1) & (sub.col == 0)))
    r, c, w = sub.row[keep].astype(np.int64), sub.col[keep].astype(np.int64), sub.data[keep]
    o = np.lexsort((c, r))
    return r[o], c[o], w[o], len(nodes)


def _dist_from(r, c, n, start, removed=None, extra=None):
    """Unweighted distances on the undirected graph (r, c) from `start`, with node `removed` taken out and
    `extra` = (a, b) added as an edge; inf where not reached."""
    rr, cc = list(r), list(c)
    if extra is not None:
        rr.append(extra[0])
        cc.append(extra[1])
    M = ssp.csr_matrix((np.ones(len(rr)), (np.asarray(rr, dtype=np.int64), np.asarray(cc, dtype=np.int64))),
                       shape=(n, n))
    if removed is not None:
        keep = np.ones(n, dtype=bool)
        keep[removed] = False
        idx = np.flatnonzero(keep)
        d = np.full(n, np.inf)
        d[idx] = shortest_path(M[idx][:, idx], directed=False, unweighted=True,
                               indices=int(np.searchsorted(idx, start)))
        return d
    return shortest_path(M, directed=False, unweighted=True, indices=start)


def label_subgraph(A, nodes, dists, label):
    r, c, w, n = induced(A, nodes)
    edges = np.stack([r, c, np.asarray(w).astype(np.int64)], axis=1) if len(r) else np.zeros((0, 3), np.int64)
    dists = np.asarray(dists, dtype=np.int64)
    if label in ("drnl", "de+"):
        ds = _dist_from(r, c, n, 0, removed=1)
        dd = _dist_from(r, c, n, 1, removed=0)
        ds[1] = 0.0
        dd[0] = 0.0
        if label == "de+":
            return edges, np.minimum(np.stack([ds, dd], 1), 100).astype(np.int64)
        with np.errstate(invalid="ignore"):
            D = ds + dd
            h = np.floor(D / 2)
            z = 1 + np.minimum(ds, dd) + h * (h + np.mod(D, 2) - 1)
        z[:2] = 1
        z[~np.isfinite(z)] = 0
        return edges, z.astype(np.int64)
    if label == "de":
        ds = _dist_from(r, c, n, 0, extra=(0, 1))
        dd = _dist_from(r, c, n, 1, extra=(0, 1))
        return edges, np.minimum(np.stack([ds, dd], 1), 3).astype(np.int64)
    if label == "hop":
        return edges, dists
    if label == "zo":
        return edges, (dists == 0).astype(np.int64)
    if label == "degree":
        z = np.zeros(n, dtype=np.int64)
        np.add.at(z, c, np.asarray(w).astype(np.int64))
        return edges, np.minimum(z, 100)
    return edges, np.zeros(n, dtype=np.int64)


def ragged(blob, key, i):
    off = blob[key + "_off"]
    return blob[key][off[i]:off[i + 1]]


def tag(label):
    return {"de+": "deplus"}.get(label, label)
