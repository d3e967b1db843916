"""fp64 numpy / scipy restatement of the link heuristics (reference utils.py CN / AA / PPR, PPR as fast_pagerank
0.0.4 `pagerank_power`), the yardstick of tests/test_heuristics_host.py and tests/test_gpu_heuristics.py.

PPR comes in two forms: `pagerank_power`, one source at a time exactly as the formula reads, and `ppr_batched`,
the sources as columns of one [N, S] block with a stop per column.  The batched form keeps the per-column
arithmetic of the loop (the same sparse mat-vec order, zᵀx and the norm per column), so the two agree."""
import numpy as np
import scipy.sparse as ssp


def canonical(A):
    A = ssp.csr_matrix(A, copy=True)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A


def cn(A, links):
    A = canonical(A)
    s, d = np.asarray(links[0]), np.asarray(links[1])
    if len(s) == 0:
        return np.zeros(0, dtype=np.float32)
    return np.asarray(A[s].multiply(A[d]).sum(1)).ravel().astype(np.float32)


def aa_weights(A):
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / np.log(np.asarray(canonical(A).sum(axis=0), dtype=np.float64).ravel())
    w[np.isinf(w)] = 0.0
    return w


def aa(A, links):
    A = canonical(A)
    s, d = np.asarray(links[0]), np.asarray(links[1])
    if len(s) == 0:
        return np.zeros(0, dtype=np.float32)
    A_ = ssp.csr_matrix(A.multiply(aa_weights(A)[None, :]))
    return np.asarray(A[s].multiply(A_[d]).sum(1)).ravel().astype(np.float32)


def _operators(A, p):
    A = canonical(A)
    n = A.shape[0]
    r = np.asarray(A.sum(axis=1)).reshape(-1)
    k = r.nonzero()[0]
    D_1 = ssp.csr_matrix((1 / r[k], (k, k)), shape=(n, n))
    W = ssp.csr_matrix(p * A.T @ D_1)
    z_T = (((1 - p) * (r != 0) + (r == 0)) / n)[np.newaxis, :]
    return W, z_T, n


def pagerank_power(A, source, p=0.85, tol=1e-7, max_iter=100, ops=None):
    """One source: (normalised x [N] fp64, iterations run)."""
    W, z_T, n = ops if ops is not None else _operators(A, p)
    s = np.zeros((n, 1))
    s[source] = n
    x, oldx = s, np.zeros((n, 1))
    it = 0
    while np.linalg.norm(x - oldx) > tol:
        oldx = x
        x = W @ x + s @ (z_T @ x)
        it += 1
        if it >= max_iter:
            break
    x = x / sum(x)
    return x.reshape(-1), it


def ppr_loop(A, sources, p=0.85, tol=1e-7, max_iter=100):
    """{source: (x [N], iterations)} by the literal per-source loop."""
    ops = _operators(A, p)
    return {int(s): pagerank_power(A, int(s), p, tol, max_iter, ops) for s in np.unique(sources)}


def ppr_batched(A, sources, p=0.85, tol=1e-7, max_iter=100):
    """(X [N, S] normalised, iterations [S]) for the distinct `sources` in the given order: every column iterates
    until its own stop, frozen columns keep their last iterate."""
    W, z_T, n = _operators(A, p)
    sources = np.asarray(sources, dtype=np.int64)
    S = len(sources)
    X = np.zeros((n, S))
    X[sources, np.arange(S)] = n
    s_col = X.copy()
    old = np.zeros((n, S))
    its = np.zeros(S, dtype=np.int64)
    active = np.array([np.linalg.norm(X[:, c:c + 1] - old[:, c:c + 1]) > tol for c in range(S)], dtype=bool)
    while active.any():
        cols = np.nonzero(active)[0]
        Xa = X[:, cols]
        t = np.array([(z_T @ Xa[:, j:j + 1])[0, 0] for j in range(len(cols))])
        Xn = W @ Xa + s_col[:, cols] * t[None, :]
        its[cols] += 1
        for j, c in enumerate(cols):
            if not np.linalg.norm(Xn[:, j:j + 1] - Xa[:, j:j + 1]) > tol or its[c] >= max_iter:
                active[c] = False
        X[:, cols] = Xn
    return X / np.array([sum(X[:, c:c + 1])[0] for c in range(S)])[None, :], its


def ppr_scores(A, links, p=0.85, tol=1e-7, max_iter=100):
    """(fp32 scores [L] in the links' order, iterations [L] of each link's source) via the batched form."""
    links = np.asarray(links, dtype=np.int64)
    if links.shape[1] == 0:
        return np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)
    src, inv = np.unique(links[0], return_inverse=True)
    X, its = ppr_batched(A, src, p, tol, max_iter)
    inv = inv.reshape(-1)
    return X[links[1], inv].astype(np.float32), its[inv]


def ppr_dense(A, source, p=0.85):
    """The converged answer: the normalised solution of (I − W)·x = e_s (W's columns sum to at most p < 1)."""
    W, _, n = _operators(A, p)
    e = np.zeros(n)
    e[source] = 1.0
    x = np.linalg.solve(np.eye(n) - W.toarray(), e)
    return x / x.sum()
