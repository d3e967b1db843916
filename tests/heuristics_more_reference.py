"""fp64 numpy / scipy restatement of the four link indices the reference does not have (DESIGN.md §23 is their
specification): resource allocation, structural Jaccard, preferential attachment and truncated Katz.  The yardstick
of tests/test_heuristics_more_host.py and tests/test_gpu_heuristics_more.py.

With `A` canonical (square CSR, duplicates summed, explicit zeros dropped, rows sorted, fp64), r its row sums, c its
column sums (added in ascending row order) and deg(i) the stored entries of row i:

    RA(s, d)      = Σ_k A[s,k]·(A[d,k]·v_k),  v_k = 1/c_k, 0 where c_k = 0
    JACCARD(s, d) = |keys(s) ∩ keys(d)| / (deg(s) + deg(d) − |∩|), 0 when that is 0
    PA(s, d)      = r_s·r_d
    KATZ(s, d)    = x_max_len[d],  x_0 = 0,  x_l[j] = β·Σ_i A[i,j]·(x_{l−1}[i] + [i = s])   (= Σ_l β^l·(A^l)[s,d])

Every sum is a scipy CSR product, which adds a row's entries one after the other in stored order: ascending keys
for a row of A, ascending i for a column of A (a row of Aᵀ), the orders the kernels use.  `Sums(rng)` stores every
row in a random order first, so the same sums are formed in another order; `Sums()` changes nothing.

`fault` selects one of the named wrong variants of `FAULTS`; the tests show that each one leaves the bounds."""
import numpy as np
import scipy.sparse as ssp

from heuristics_reference import canonical

FAULTS = ("ra_row_sums", "ra_zero_column_inf", "jaccard_no_minus", "jaccard_on_values", "pa_column_sums",
          "katz_no_transpose", "katz_no_last_level", "katz_source_first_level_only", "katz_beta_once",
          "walk_drops_last_entry", "finish_reads_buffer_0")


class Sums:
    """How sums are formed: in stored order, or with rng in a random order of every sum's terms."""

    def __init__(self, rng=None):
        self.rng = rng

    def ordered(self, M):
        """M as CSR, its rows' entries in stored order or, with rng, shuffled inside every row"""
        M = ssp.csr_matrix(M)
        if self.rng is None or M.nnz == 0:
            return M
        rows = np.repeat(np.arange(M.shape[0]), np.diff(M.indptr))
        order = np.lexsort((self.rng.random(M.nnz), rows))
        return ssp.csr_matrix((M.data[order], M.indices[order], M.indptr), shape=M.shape)

    def rows(self, M):
        """Σ over every row of M: [rows] fp64"""
        return np.asarray(self.ordered(M) @ np.ones(M.shape[1])).reshape(-1)

    def mm(self, M, X):
        """M @ X for dense X [cols, k]"""
        return np.asarray(self.ordered(M) @ X)


def _fp64(A):
    A = canonical(A)
    return ssp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)


def _transpose(A):
    """Aᵀ as CSR with sorted rows: row j lists the i with A[i, j] stored, ascending"""
    T = ssp.csr_matrix(A.T)
    T.sort_indices()
    return T


def row_sums(A, sums=None):
    return (sums or Sums()).rows(_fp64(A))


def column_sums(A, sums=None):
    return (sums or Sums()).rows(_transpose(_fp64(A)))


def ra_weights(A, sums=None, fault=None):
    A = _fp64(A)
    c = row_sums(A, sums) if fault == "ra_row_sums" else column_sums(A, sums)
    with np.errstate(divide="ignore"):
        v = 1.0 / c
    if fault != "ra_zero_column_inf":
        v[c == 0] = 0.0
    return v


def _links(links):
    links = np.asarray(links, dtype=np.int64)
    return links[0], links[1]


def _walked_last(A, s, d):
    """per link, the last key of the row pairs_kernel walks (the shorter; a tie: the smaller id), -1 for an empty one"""
    deg = np.diff(A.indptr)
    walk_s = (deg[s] < deg[d]) | ((deg[s] == deg[d]) & (s <= d))
    w = np.where(walk_s, s, d)
    return np.where(deg[w] > 0, A.indices[np.maximum(A.indptr[w + 1] - 1, 0)], -1)


def _common(A, B, s, d, fault):
    """CSR [L, N] of the terms A[s,k]·B[d,k] over the common keys"""
    with np.errstate(invalid="ignore", over="ignore"):
        M = ssp.csr_matrix(A[s].multiply(B[d]))
    if fault == "walk_drops_last_entry":
        M = M.tolil()
        for l, k in enumerate(_walked_last(A, s, d)):
            if k >= 0:
                M[l, k] = 0.0
        M = ssp.csr_matrix(M)
    return M


def ra(A, links, sums=None, fault=None, with_magnitude=False, dtype=np.float32):
    """RA of every link; with_magnitude also returns Σ_k |term| per link (fp64)"""
    A, sums = _fp64(A), sums or Sums()
    s, d = _links(links)
    if len(s) == 0:
        z = np.zeros(0, dtype=dtype)
        return (z, np.zeros(0)) if with_magnitude else z
    v = ra_weights(A, sums, fault)
    with np.errstate(invalid="ignore", over="ignore"):
        B = ssp.csr_matrix((A.data * v[A.indices], A.indices, A.indptr), shape=A.shape)   # a_dk·v_k, zeros kept
        M = _common(A, B, s, d, fault)
        out = sums.rows(M).astype(dtype)
    return (out, sums.rows(abs(M))) if with_magnitude else out


def jaccard(A, links, sums=None, fault=None, dtype=np.float32):
    A, sums = _fp64(A), sums or Sums()
    s, d = _links(links)
    if len(s) == 0:
        return np.zeros(0, dtype=dtype)
    if fault == "jaccard_on_values":       # the weighted form: Σ a_s·a_d over (r_s + r_d − Σ a_s·a_d)
        P, size = A, row_sums(A, sums)
    else:
        P = ssp.csr_matrix((np.ones(A.nnz), A.indices, A.indptr), shape=A.shape)
        size = np.diff(A.indptr).astype(np.float64)
    both = sums.rows(_common(P, P, s, d, fault))
    either = size[s] + size[d] - (0.0 if fault == "jaccard_no_minus" else both)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = np.where(either != 0, both / either, 0.0)
    return out.astype(dtype)


def pa(A, links, sums=None, fault=None, dtype=np.float32):
    s, d = _links(links)
    r = column_sums(A, sums) if fault == "pa_column_sums" else row_sums(A, sums)
    return (r[s] * r[d]).astype(dtype)


def katz_columns(A, sources, beta=0.005, max_len=3, sums=None, fault=None):
    """X [N, S] fp64: column k is x_max_len of sources[k]"""
    A, sums = _fp64(A), sums or Sums()
    n = A.shape[0]
    sources = np.asarray(sources, dtype=np.int64)
    T = A if fault == "katz_no_transpose" else _transpose(A)
    E = np.zeros((n, len(sources)))
    E[sources, np.arange(len(sources))] = 1.0
    levels = max_len - 1 if fault == "katz_no_last_level" else max_len
    scale = 1.0 if fault == "katz_beta_once" else beta
    buf = [np.zeros((n, len(sources))), np.zeros((n, len(sources)))]    # level l writes buffer l & 1
    with np.errstate(over="ignore", invalid="ignore"):
        for level in range(1, levels + 1):
            x = buf[(level - 1) & 1]
            operand = x + E if (level == 1 or fault != "katz_source_first_level_only") else x
            buf[level & 1] = scale * sums.mm(T, operand)
        X = buf[0] if fault == "finish_reads_buffer_0" else buf[levels & 1]
        return beta * X if fault == "katz_beta_once" else X


def katz(A, links, beta=0.005, max_len=3, sums=None, fault=None, dtype=np.float32):
    """Katz of every link, in the links' order; each distinct source solved once"""
    s, d = _links(links)
    if len(s) == 0:
        return np.zeros(0, dtype=dtype)
    src, inv = np.unique(s, return_inverse=True)
    inv, out = inv.reshape(-1), np.zeros(len(s))
    for a in range(0, len(src), 1024):                    # dense [N, 1024] blocks: memory only, a column stands alone
        mine = (inv >= a) & (inv < a + 1024)
        out[mine] = katz_columns(A, src[a:a + 1024], beta, max_len, sums, fault)[d[mine], inv[mine] - a]
    with np.errstate(over="ignore"):
        return out.astype(dtype)


def max_column_entries(A):
    A = _fp64(A)
    return int(np.bincount(A.indices, minlength=A.shape[1]).max()) if A.nnz else 0


def ulp32(ref):
    return np.spacing(np.abs(np.asarray(ref, dtype=np.float32))).astype(np.float64)


def katz_noise(A, links, beta, max_len):
    """The fp64 part of the Katz bound, per score: 2·max_len·(m + 3)·2⁻⁵³·KATZ_{|A|,|β|}(s, d), m the largest
    stored-entry count of a column.  First-order worst case of max_len dot products of at most m terms, each
    followed by one add and one multiply; the factor 2 covers the higher-order terms."""
    A = _fp64(A)
    mag = katz(abs(A), links, abs(beta), max_len, dtype=np.float64)
    return 2.0 * max_len * (max_column_entries(A) + 3) * 2.0 ** -53 * mag


def katz_bound(A, links, beta, max_len):
    """1 fp32 ulp of the restatement + katz_noise"""
    return ulp32(katz(A, links, beta, max_len)) + katz_noise(A, links, beta, max_len)
