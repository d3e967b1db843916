"""Graphs, link lists and segment lists for the NCN tests (tests/test_ncn_host.py, tests/test_gpu_ncn.py; DESIGN.md
§26).  numpy and scipy only; everything is deterministic from fixed seeds.

    list_cases()      name -> (A, links): the 300-node symmetric graph and the 40-node directed one of
                      `sketch_mask_cases`, `sketch_cases.hub_graph` with its links, and `length_graph`
    length_graph()    rows of every length of LENGTHS twice: node k holds the first LENGTHS[k] keys of a pool (so against
                      a longer row EVERY position of the walked row survives: first, last, both sides of each 64-key
                      boundary), node 10 + k a random subset of the pool of the same length (so some survive).  Some
                      rows hold their own id and their partner's, for the flag.  Links: all ordered pairs, u == v too
    prefix_links(n)   the first n links of a list that starts at the hub graph's two long rows: 0, 1, 2, 3, 5, 11
    segment_case()    (M, ptr, idx): segments of every length of SEGMENTS in an order that puts long and short rows in
                      one workgroup, one of them 300 repeats of one row
    autograd_case()   (A, links): the hub graph with 200 links of its own rows, and four hubs adjacent to the endpoints
                      of 325 more links, so that nodes are the common neighbour of 0, 1, 64, 65 and 325 links
"""
from functools import lru_cache

import numpy as np
import scipy.sparse as ssp

import sketch_cases as K
import sketch_mask_cases as MC

LENGTHS = (0, 1, 2, 63, 64, 65, 128, 129, 600)
SEGMENTS = (0, 1, 63, 64, 65, 127, 128, 129, 256, 257, 4097)
WIDTHS = (1, 3, 4, 5, 32, 33, 256, 260)
LIST_SIZES = (0, 1, 2, 3, 5, 11)


@lru_cache(maxsize=None)
def length_graph():
    rng = np.random.default_rng(26)
    n, pool = 800, np.arange(30, 800)
    rows = [[] for _ in range(n)]
    # (node, the small ids its row holds besides pool keys): self-loops and partners, for exclude_endpoints
    extra = {4: [4, 14], 14: [4, 14], 5: [5], 16: [6], 6: [16], 8: [8, 18], 18: [8], 7: [17]}
    for k, d in enumerate(LENGTHS):
        for node, keys in ((k, pool[:d]), (10 + k, np.sort(rng.choice(pool[:700], d, replace=False)))):
            own = [x for x in extra.get(node, [])][:d]
            rows[node] = own + keys[:d - len(own)].tolist()
    for x in pool:
        rows[x] = rng.choice(pool, int(rng.integers(0, 4)), replace=False).tolist()
    A = MC._csr([sorted(set(r)) for r in rows], n)
    deg = np.diff(A.indptr)
    assert deg[:9].tolist() == list(LENGTHS) and deg[10:19].tolist() == list(LENGTHS)
    special = np.r_[0:9, 10:19]
    u, v = np.meshgrid(special, special, indexing="ij")
    return A, np.stack([u.reshape(-1), v.reshape(-1)]).astype(np.int64)


@lru_cache(maxsize=None)
def hub_case():
    """the hub graph with its own links, the two long rows first and repeated, and a link at the isolated node"""
    A, links = K.hub_graph()
    head = np.array([[0, 1, 0, 2, 2, 0, 1], [1, 0, 1, 0, 2, 0, 1]], dtype=np.int64)
    return A, np.concatenate([head, links], axis=1)


def list_cases():
    return {"random": MC.random_case(), "directed": MC.directed_case(), "hub": hub_case(), "lengths": length_graph()}


def prefix_links(n):
    A, links = hub_case()
    return A, links[:, :n].copy()


def dense_lists(A, links, exclude_endpoints):
    """the lists from a dense (A[u] & A[v]) mask, one link at a time"""
    D = np.asarray(ssp.csr_matrix(A).todense()) != 0
    out = []
    for u, v in np.asarray(links).T.tolist():
        m = D[u] & D[v]
        if exclude_endpoints:
            m = m.copy()
            m[[u, v]] = False
        out.append(np.nonzero(m)[0])
    return out


def without_link(A, u, v):
    """A without the stored entries (u, v) and (v, u)"""
    B = ssp.lil_matrix(ssp.csr_matrix(A, copy=True))
    B[u, v] = 0
    B[v, u] = 0
    B = ssp.csr_matrix(B)
    B.eliminate_zeros()
    return B


@lru_cache(maxsize=None)
def segment_case():
    """M = 500 source rows.  The order puts the 4 097-entry row beside empty and short rows in the first workgroup, two
    long rows in one workgroup, and a workgroup of short rows only; the last segment repeats row 7 300 times."""
    rng = np.random.default_rng(4097)
    M = 500
    order = (4097, 0, 1, 63, 257, 256, 64, 129, 65, 127, 128, 0, 2)
    assert set(SEGMENTS) <= set(order)
    segs = [rng.integers(0, M, d) for d in order] + [np.full(300, 7)]
    ptr = np.r_[0, np.cumsum([len(s) for s in segs])].astype(np.int64)
    return M, ptr, np.concatenate(segs).astype(np.int32)


def first_rows(ptr, idx, R):
    return ptr[:R + 1].copy(), idx[:ptr[R]].copy()


HUBS = (900, 901, 902, 903, 904)    # common neighbour of 325, 65, 64, 1 and 0 links of autograd_case


@lru_cache(maxsize=None)
def autograd_case():
    base, own = K.hub_graph()
    rng = np.random.default_rng(325)
    n = 950
    P, Q = np.arange(905, 930), np.arange(930, 943)             # 25 x 13 = 325 links
    rows = [base.indices[base.indptr[x]:base.indptr[x + 1]].tolist() for x in range(900)] + [[] for _ in range(n - 900)]
    for x in np.r_[P, Q]:
        rows[x] = [900] + rng.choice(np.arange(5, 900), 3, replace=False).tolist()
    for x in np.r_[P[:5], Q]:
        rows[x].append(901)                                     # 5 x 13 = 65 links
    for x in np.r_[P[5:13], Q[:8]]:
        rows[x].append(902)                                     # 8 x 8 = 64 links
    rows[P[20]].append(903)
    rows[Q[12]].append(903)                                     # one link
    A = MC._csr([sorted(set(r)) for r in rows], n)
    extra = rng.integers(0, 900, size=(2, 200 - own.shape[1]))
    u, v = np.meshgrid(P, Q, indexing="ij")
    links = np.concatenate([own, extra, np.stack([u.reshape(-1), v.reshape(-1)])], axis=1).astype(np.int64)
    assert own.shape[1] + extra.shape[1] == 200
    return A, links[:, rng.permutation(links.shape[1])]
