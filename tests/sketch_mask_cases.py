"""Graphs and link lists for the masked-sketch tests (tests/test_sketch_mask_host.py, tests/test_gpu_sketch_mask.py;
DESIGN.md §25).  numpy and scipy only; everything is deterministic from fixed seeds.  Every case is (A, links) with
links int64 [2, L]; a link is `stored` one way when (u, v) is an entry of A and (v, u) is not.

    random_case()     the 300-node symmetric graph at mean degree 4: 24 edges (stored both ways), 7 non-edges and a
                      link at an isolated node, 32 links in all
    directed_case()   40 nodes, directed: links stored both ways, one way in either orientation and not at all, u == v
                      with and without a self-loop, an endpoint with a self-loop, a degree-1 endpoint whose only key
                      is the partner, an isolated node
    length_case()     masked endpoints whose rows hold 0, 1, 2, 3, 4, 5, 63, 64 and 65 keys, the partner first or last
    hub_case()        `sketch_cases.hub_graph` and its links, plus the 600-key and the 260-key row with the partner at
                      every position of `quarter_positions`
    long_case()       `sketch_cases.hub_graph` with the two long rows (601 and 261 keys) pointing at each other and
                      some short rows pointing back at the hub: the partner at the first and last key, inside every
                      wavefront's quarter and on both sides of every quarter boundary; both endpoints long, one long
"""
from functools import lru_cache

import numpy as np
import scipy.sparse as ssp

import sketch_cases as K

SPLIT_KEYS, WAVES = 64, 4     # kSplitKeys and kSkWaves of csrc/s3grl_sketch.hip


def _csr(rows, n):
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    cols = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if indptr[-1] else np.zeros(0, np.int64)
    A = ssp.csr_matrix((np.ones(indptr[-1]), cols.astype(np.int32), indptr), shape=(n, n))
    A.sort_indices()
    return A


def stored(A, links):
    """bool [2, L]: whether (u, v) and whether (v, u) is an entry of A"""
    A = ssp.csr_matrix(A)
    u, v = np.asarray(links, dtype=np.int64).reshape(2, -1)
    return np.stack([np.asarray(A[u, v]).reshape(-1) != 0, np.asarray(A[v, u]).reshape(-1) != 0])


@lru_cache(maxsize=None)
def random_case():
    A = K.random_symmetric(300, 4, seed=300)
    rng = np.random.default_rng(301)
    coo = A.tocoo()
    at = rng.choice(A.nnz, 24, replace=False)
    u = rng.integers(0, 300, 7)
    v = (u + rng.integers(1, 300, 7)) % 300
    free = np.asarray(A[u, v]).reshape(-1) == 0
    lonely = np.nonzero(np.diff(A.indptr) == 0)[0]
    assert free.all() and len(lonely), "seed 300 gives seven non-edges and an isolated node"
    links = np.stack([np.r_[coo.row[at], u, lonely[0]], np.r_[coo.col[at], v, coo.row[at[0]]]]).astype(np.int64)
    return A, links


@lru_cache(maxsize=None)
def directed_case():
    rng = np.random.default_rng(40)
    n = 40
    far = np.arange(15, n)

    def some(k):
        return rng.choice(far, k, replace=False).tolist()

    rows = [[] for _ in range(n)]
    rows[0] = [1] + some(3)                 # (0, 1) stored, (1, 0) not
    rows[1] = some(4)
    rows[2] = [3] + some(2)                 # (2, 3) and (3, 2) stored
    rows[3] = [2] + some(5)
    rows[4], rows[5] = some(3), some(2)     # (4, 5) not stored either way
    rows[6] = [6] + some(3)                 # u == v on a self-loop
    rows[7] = some(3)                       # u == v without one
    rows[8] = [8, 9] + some(2)              # an endpoint with a self-loop, stored both ways
    rows[9] = [8] + some(3)
    rows[10] = [11]                         # its only key is the partner: rows 1 and 2 fall back to row 0
    rows[11] = [10, 12, 13]
    rows[12], rows[13] = some(2), [12]
    # row 14 stays empty and nobody points at 14: isolated
    for x in far:
        rows[x] = rng.choice(np.r_[0:14, far], int(rng.integers(0, 6)), replace=False).tolist()
    A = _csr([sorted(set(r)) for r in rows], n)
    pairs = [(0, 1), (1, 0), (2, 3), (3, 2), (4, 5), (6, 6), (7, 7), (8, 9), (9, 8), (8, 8), (10, 11), (11, 10),
             (14, 0), (0, 14), (14, 14), (11, 12), (13, 12), (12, 13)]
    for x in far[:6]:                       # stored entries among the random rows, in both orders
        if A.indptr[x + 1] > A.indptr[x]:
            w = int(A.indices[A.indptr[x]])
            pairs += [(int(x), w), (w, int(x))]
    return A, np.array(pairs, dtype=np.int64).T.copy()


LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65)


@lru_cache(maxsize=None)
def length_case():
    """Node k (k < 9) has LENGTHS[k] keys, one of them its partner 10 + k (the first key) for the short rows and
    390 + k (the last key) for the three long ones; the partner points back for even k.  The node without keys is
    masked from its partner's side only."""
    rng = np.random.default_rng(65)
    n = 400
    other = np.arange(20, 390)
    rows = [[] for _ in range(n)]
    pairs = []
    for k, d in enumerate(LENGTHS):
        y = 10 + k if d < 63 else 390 + k
        rows[k] = ([y] if d else []) + rng.choice(other, max(d - 1, 0), replace=False).tolist()
        rows[y] = rng.choice(other, 2, replace=False).tolist() + ([k] if k % 2 == 0 else [])
        pairs += [(k, y), (y, k)]
    for x in other:
        rows[x] = rng.choice(other, int(rng.integers(0, 5)), replace=False).tolist()
    A = _csr([sorted(set(r)) for r in rows], n)
    assert np.diff(A.indptr)[:9].tolist() == list(LENGTHS)
    return A, np.array(pairs, dtype=np.int64).T.copy()


def quarter_positions(deg):
    """Positions in a row of `deg` > SPLIT_KEYS keys: first, last, the middle of every wavefront's share and both
    sides of every boundary between two shares."""
    share = -(-deg // WAVES)
    at = {0, deg - 1}
    for q in range(WAVES):
        at.add(min(deg - 1, q * share + share // 2))
        if q:
            at.update((q * share - 1, min(deg - 1, q * share)))
    return sorted(at)


@lru_cache(maxsize=None)
def long_case():
    base, _ = K.hub_graph()
    A = ssp.lil_matrix(base)
    A[0, 1] = 1.0
    A[1, 0] = 1.0
    row0 = np.sort(np.r_[base.indices[base.indptr[0]:base.indptr[1]], 1])
    row1 = np.sort(np.r_[base.indices[base.indptr[1]:base.indptr[2]], 0])
    at0, at1 = quarter_positions(len(row0)), quarter_positions(len(row1))
    back = [int(row0[p]) for p in at0[2::3]]          # these short rows point back at the hub: one long, one short
    for w in back:
        A[w, 0] = 1.0
    A = ssp.csr_matrix(A)
    A.sort_indices()
    assert np.diff(A.indptr)[:2].tolist() == [601, 261] and np.diff(A.indptr)[back].max() <= SPLIT_KEYS
    pairs = [(0, 1), (1, 0)]                          # both endpoints long
    pairs += [(0, int(row0[p])) for p in at0] + [(int(row0[p]), 0) for p in at0]
    pairs += [(1, int(row1[p])) for p in at1]
    pairs += [(0, 2), (3, 0), (0, 0), (7, 1)]         # long rows that hold no entry of the link: the table rows
    return A, np.array(pairs, dtype=np.int64).T.copy()


@lru_cache(maxsize=None)
def hub_case():
    """`sketch_cases.hub_graph` as it is (directed: nobody points at rows 0 and 1) with its own links and, for the
    600-key and the 260-key row, the partner at every position of `quarter_positions`, in both orders: one endpoint
    long and masked, the other short and not."""
    A, links = K.hub_graph()
    pairs = []
    for x in (0, 1):
        row = A.indices[A.indptr[x]:A.indptr[x + 1]]
        pairs += [(x, int(row[p])) for p in quarter_positions(len(row))]
    pairs = np.array(pairs + [(v, u) for u, v in pairs], dtype=np.int64).T
    return A, np.concatenate([links, pairs], axis=1)


def every_case():
    return {"random": random_case(), "directed": directed_case(), "lengths": length_case(), "hub": hub_case(),
            "long": long_case()}
