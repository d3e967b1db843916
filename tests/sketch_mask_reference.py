"""numpy restatement of the masked subgraph sketches (`sketch_masked_pairs_kernel` in
csrc/s3grl_sketch.hip), for tests/test_sketch_mask_host.py and tests/test_gpu_sketch_mask.py.

The masked outputs of a link (u, v) are what tests/sketch_reference.py gives for it on the graph without the stored
entries (u, v) and (v, u).  For hops <= 2 no row other than u's and v's loses an entry, so they follow from the tables
of the unmasked graph: with x one endpoint, y the other and (x, y) stored,

    MH'_1[x] = min(MH_0[x], min of MH_0[w] over w in row(x), w != y)
    MH'_2[x] = min(MH'_1[x], min of MH_1[w] over w in row(x), w not in {x, y})

and HL' the same with max; an endpoint whose entry is not stored keeps its table rows.  A self-loop w = x would
contribute MH'_1[x], which is already in, and must not contribute the table's MH_1[x], which holds y.

    masked_rows(indptr, indices, mh, hl, x, y)              # uint32 [hops+1, P], uint8 [hops+1, m] of endpoint x
    masked_link_outputs(A, mh, hl, links, hll_p)            # match, T, z, intersections, features as the device stores
    without_link(A, u, v)                                   # the graph the masked outputs of (u, v) describe
    rebuilt_link_outputs(A, links, hops, P, hll_p, seed)    # one `sketch_reference.sketches` per link: the definition

`fault` names one deliberate departure (FAULTS); the host test shows that each of them breaks the byte equality.
"""
import numpy as np
import scipy.sparse as ssp

import sketch_reference as R

FAULTS = ("partner_kept_hop1", "partner_kept_hop2", "own_hop1_left_out")
NAMES = ("match", "T", "z", "intersections", "features")


def _reduce(op, start, rows):
    return op(start, op.reduce(rows, axis=0)) if len(rows) else start


def masked_rows(indptr, indices, mh, hl, x, y, fault=None):
    """The rows of endpoint x on the graph without (x, y): the table rows when (x, y) is not stored."""
    K = mh.shape[0]
    if K > 3:
        raise NotImplementedError("the closed form holds for hops <= 2")
    row = indices[indptr[x]:indptr[x + 1]]
    if y not in row:
        return mh[:, x], hl[:, x]
    m, h = mh[:, x].copy(), hl[:, x].copy()
    w1 = row if fault == "partner_kept_hop1" else row[row != y]
    m[1], h[1] = _reduce(np.minimum, m[0], mh[0][w1]), _reduce(np.maximum, h[0], hl[0][w1])
    if K == 3:
        w2 = row[row != x] if fault == "partner_kept_hop2" else row[(row != x) & (row != y)]
        if fault == "own_hop1_left_out":
            m[2] = _reduce(np.minimum, np.full_like(m[1], 0xFFFFFFFF), mh[1][w2])
            h[2] = _reduce(np.maximum, np.zeros_like(h[1]), hl[1][w2])
        else:
            m[2], h[2] = _reduce(np.minimum, m[1], mh[1][w2]), _reduce(np.maximum, h[1], hl[1][w2])
    return m, h


def masked_link_outputs(A, mh, hl, links, hll_p, fault=None):
    """`sketch_reference.link_outputs` with every link's own stored entries masked, from the unmasked tables."""
    indptr, indices = R._csr(A)
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    K, L, P = mh.shape[0], links.shape[1], mh.shape[2]
    mu, mv = mh[:, links[0]].transpose(1, 0, 2).copy(), mh[:, links[1]].transpose(1, 0, 2).copy()   # [L, K, P]
    hu, hv = hl[:, links[0]].transpose(1, 0, 2).copy(), hl[:, links[1]].transpose(1, 0, 2).copy()   # [L, K, m]
    n = len(indptr) - 1
    keys = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr)) * n + indices                   # ascending
    for (x, y), (m_out, h_out) in (((links[0], links[1]), (mu, hu)), ((links[1], links[0]), (mv, hv))):
        for l in np.nonzero(np.isin(x * n + y, keys))[0]:
            m_out[l], h_out[l] = masked_rows(indptr, indices, mh, hl, int(x[l]), int(y[l]), fault)
    match = np.zeros((L, K, K), dtype=np.int32)
    T = np.zeros((L, K, K), dtype=np.int64)
    z = np.zeros((L, K, K), dtype=np.int32)
    for i in range(K):
        for j in range(K):
            match[:, i, j] = (mu[:, i] == mv[:, j]).sum(axis=1)
            T[:, i, j], z[:, i, j] = R.tz(np.maximum(hu[:, i], hv[:, j]), hll_p)
    I = R.intersections(match, T, z, P, hll_p)
    F = R.features(I, R.cardinality(hu, hll_p), R.cardinality(hv, hll_p))
    return {"match": match, "T": T, "z": z, "intersections": I.astype(np.float32), "features": F.astype(np.float32)}


def without_link(A, u, v):
    """A without the stored entries (u, v) and (v, u), whichever of them there are."""
    A = ssp.lil_matrix(ssp.csr_matrix(A, copy=True))
    A[u, v] = 0
    A[v, u] = 0
    A = ssp.csr_matrix(A)
    A.eliminate_zeros()
    return A


def rebuilt_link_outputs(A, links, hops, num_perm, hll_p, seed=0):
    """The definition: every link's outputs from `sketch_reference.sketches` of the graph without that link."""
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    out = {k: [] for k in NAMES}
    for u, v in links.T:
        mh, hl = R.sketches(without_link(A, int(u), int(v)), hops, num_perm, hll_p, seed)
        one = R.link_outputs(mh, hl, np.array([[u], [v]]), hll_p)
        for k in NAMES:
            out[k].append(one[k])
    return {k: np.concatenate(v, axis=0) for k, v in out.items()}
