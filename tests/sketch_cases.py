"""Graphs and link lists for the subgraph-sketch tests (tests/test_sketch_host.py, tests/test_gpu_sketch.py).  numpy
and scipy only; everything is deterministic from fixed seeds.

    random_symmetric(n, deg, seed)   an undirected random graph of about n·deg/2 edges, unit weights
    accuracy_case(n, deg)            that graph with 2 000 links, half of them stored entries
    order_case()                     (A, links, hops, P, p) on which the ORDER of the inclusion-exclusion shows in fp32
    hub_graph()                      a 600-key hub row among short rows, an isolated node and a self-loop, directed
"""
from functools import lru_cache

import numpy as np
import scipy.sparse as ssp


def random_symmetric(n, mean_degree, seed):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, n, size=(n * mean_degree // 2, 2))
    e = e[e[:, 0] != e[:, 1]]
    A = ssp.csr_matrix((np.ones(2 * len(e)), (np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]])), shape=(n, n))
    A.sum_duplicates()
    A.data[:] = 1.0
    return A


@lru_cache(maxsize=None)
def accuracy_case(n, mean_degree):
    """(A, links [2, 2000]): 1 000 stored entries of A and 1 000 random pairs u != v."""
    A = random_symmetric(n, mean_degree, seed=n)
    rng = np.random.default_rng(n + 1)
    coo = A.tocoo()
    at = rng.choice(A.nnz, 1000, replace=False)
    u = rng.integers(0, n, 1000)
    v = (u + rng.integers(1, n, 1000)) % n
    return A, np.stack([np.r_[coo.row[at], u], np.r_[coo.col[at], v]]).astype(np.int64)


@lru_cache(maxsize=None)
def order_case():
    """A reordered fp64 sum moves a result by an ulp of fp64, which the fp32 store hides unless the specified order
    cancels to exactly 0 and the other does not.  That happens where one endpoint's ball stops growing
    (I_ij = I_{i-1,j} and I_{i,j-1} = I_{i-1,j-1}): small components, several hops.  The first 8 192 ordered pairs
    of the 300-node graph at hops 4 hold such links (test_sketch_host.py asserts it)."""
    A = random_symmetric(300, 4, seed=300)
    links = np.stack(np.meshgrid(np.arange(300), np.arange(300))).reshape(2, -1)[:, :8192]
    return A, links.astype(np.int64), 4, 64, 7


@lru_cache(maxsize=None)
def hub_graph():
    """(A [900, 900] directed, links): row 0 holds 600 keys (the split-row path, 150 keys per wavefront), row 1 holds
    260 (shares of 65: a second 64-key batch of one key), row 2 is empty and nobody points at node 2 (isolated), row
    3 is a self-loop only, row 4 a self-loop and two keys; the rest are rows of 0..6 keys.  Links: the special rows
    with each other, with themselves and with random nodes, in both orders."""
    rng = np.random.default_rng(600)
    n = 900
    rows = [np.sort(rng.choice(np.arange(5, n), 600, replace=False)), np.sort(rng.choice(np.arange(5, n), 260, replace=False)),
            np.zeros(0, np.int64), np.array([3]), np.array([4, 10, 11])]
    while len(rows) < n:
        rows.append(np.sort(rng.choice(np.arange(3, n), int(rng.integers(0, 7)), replace=False)))
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    A = ssp.csr_matrix((np.ones(indptr[-1]), np.concatenate(rows).astype(np.int32), indptr), shape=(n, n))
    special = np.arange(5)
    u = np.r_[np.repeat(special, 5), special, rng.integers(0, n, 40)]
    v = np.r_[np.tile(special, 5), rng.integers(5, n, 5), rng.integers(0, n, 40)]
    links = np.stack([np.r_[u, v], np.r_[v, u]]).astype(np.int64)
    return A, links
