"""The link-recommendation kernels restated in numpy / scipy (test infrastructure): a BFS per source for the
candidates, the lexsort rule for the segment top-K.  Nothing here is shared with s3grl_amd.recommend."""
import numpy as np
import scipy.sparse as ssp


def csr_of(num_nodes, edges):
    """Undirected edges [E, 2] -> the symmetric CSR (structure only, duplicates merged)."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    r, c = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    A = ssp.csr_matrix((np.ones(len(r), dtype=np.int64), (r, c)), shape=(num_nodes, num_nodes))
    A.sum_duplicates()
    A.sort_indices()
    return A


def candidates(A, sources, hops=2, exclude=None):
    """(seg_ptr int64 [S + 1], cand int32): per occurrence of a source u, in ascending id, every v with
    2 <= dist(u, v) <= hops, less the pairs of `exclude` [2, E] in either orientation."""
    A = ssp.csr_matrix(A)
    n, indptr, indices = A.shape[0], A.indptr, A.indices
    banned = set()
    if exclude is not None:
        for a, b in np.asarray(exclude, dtype=np.int64).reshape(2, -1).T.tolist():
            banned.add((min(a, b), max(a, b)))
    seg_ptr, out = [0], []
    for u in np.asarray(sources, dtype=np.int64).reshape(-1).tolist():
        dist = np.full(n, -1, dtype=np.int64)
        dist[u] = 0
        frontier = [u]
        for d in range(1, hops + 1):
            nxt = []
            for x in frontier:
                for v in indices[indptr[x]:indptr[x + 1]].tolist():
                    if dist[v] < 0:
                        dist[v] = d
                        nxt.append(v)
            frontier = nxt
        seg = [v for v in np.nonzero(dist >= 2)[0].tolist() if (min(u, v), max(u, v)) not in banned]
        out += seg
        seg_ptr.append(len(out))
    return np.asarray(seg_ptr, dtype=np.int64), np.asarray(out, dtype=np.int32)


def segment_order(scores):
    """The positions of one segment, best first: score descending, then position ascending, -0.0 as +0.0, NaNs
    last (among themselves by position) = numpy.lexsort((position, -score)) with the NaNs moved last."""
    s = np.asarray(scores, dtype=np.float32)
    nan = np.isnan(s)
    return np.lexsort((np.arange(len(s)), -np.where(nan, np.float32(0), s), nan))


def segment_topk(scores, seg_ptr, cand, k):
    """(nodes int32 [S, k] padded with -1, scores fp32 [S, k] padded with -inf, count int32 [S])."""
    scores, cand = np.asarray(scores, dtype=np.float32), np.asarray(cand, dtype=np.int32)
    S = len(seg_ptr) - 1
    nodes = np.full((S, k), -1, dtype=np.int32)
    top = np.full((S, k), -np.inf, dtype=np.float32)
    count = np.zeros(S, dtype=np.int32)
    for i in range(S):
        a, b = int(seg_ptr[i]), int(seg_ptr[i + 1])
        order = segment_order(scores[a:b])[:k]
        count[i] = len(order)
        nodes[i, :len(order)] = cand[a:b][order]
        top[i, :len(order)] = scores[a:b][order]
    return nodes, top, count
