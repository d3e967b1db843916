"""A numpy restatement of the NCN operator (kernels in s3grl_amd/csrc/s3grl_ncn.hip), with no torch on
the hot path.  The kernels must equal it to the bit.

    cn_lists(A, links, exclude_endpoints)   (ptr int64 [L+1], idx int32) by np.intersect1d on the CSR rows
    segment_sum(h, ptr, idx)                fp32 [R, H] in the specified order of additions, as explicit loops
    transpose(ptr, idx, num_nodes)          (t_ptr int64 [N+1], t_link int32) by a stable argsort
    cn_sum(z, ptr, idx) / cn_sum_grad(g, ptr, idx, N)   the operator and its gradient in z

The order of the fp32 additions: a row is cut into chunks of CHUNK = 64 consecutive entries; a chunk's partial is the
sequential sum of its entries in ascending j starting from the chunk's first entry (not from 0.0); the row is the
sequential sum of the partials in ascending chunk order starting from the first partial; an empty row is +0.0.

`fault=` gives a named wrong variant; tests/test_ncn_host.py shows that each leaves byte equality on a case built
for it:
    "unchunked"        one plain ascending sum over the whole row
    "from_zero"        every chunk starts from 0.0, so a chunk of -0.0 entries gives +0.0
    "descending_links" the transpose lists a node's links in descending link index
"""
import numpy as np
import scipy.sparse as ssp

CHUNK = 64
FAULTS = ("unchunked", "from_zero", "descending_links")


def _rows(A):
    A = ssp.csr_matrix(A)
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64)


def cn_lists(A, links, exclude_endpoints=True):
    indptr, indices = _rows(A)
    u, v = np.asarray(links, dtype=np.int64).reshape(2, -1)
    lists = []
    for a, b in zip(u.tolist(), v.tolist()):
        common = np.intersect1d(indices[indptr[a]:indptr[a + 1]], indices[indptr[b]:indptr[b + 1]])
        if exclude_endpoints:
            common = common[(common != a) & (common != b)]
        lists.append(common)
    ptr = np.r_[0, np.cumsum([len(c) for c in lists])].astype(np.int64)
    idx = np.concatenate(lists).astype(np.int32) if len(lists) and ptr[-1] else np.zeros(0, np.int32)
    return ptr, idx


def _sequential(rows, start=None):
    """rows [k, H] fp32 added one after the other, from rows[0] itself (or from `start`)"""
    acc = rows[0].copy() if start is None else start + rows[0]
    for j in range(1, len(rows)):
        acc = acc + rows[j]
    return acc.astype(np.float32)


def segment_sum(h, ptr, idx, fault=None):
    assert fault in (None,) + FAULTS
    h = np.asarray(h, dtype=np.float32)
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    R, H = len(ptr) - 1, h.shape[1]
    out = np.zeros((R, H), dtype=np.float32)
    zero = np.zeros(H, dtype=np.float32)
    for r in range(R):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e == b:
            continue                                       # an empty row is +0.0
        rows = h[idx[b:e]]
        if fault == "unchunked":
            out[r] = _sequential(rows)
            continue
        partials = [_sequential(rows[c:c + CHUNK], zero if fault == "from_zero" else None)
                    for c in range(0, e - b, CHUNK)]
        out[r] = _sequential(np.stack(partials))
    return out


def transpose(ptr, idx, num_nodes, fault=None):
    """per node w the links whose list holds w, in ascending link index"""
    assert fault in (None,) + FAULTS
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    owner = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))
    order = np.argsort(idx, kind="stable")
    t_link = owner[order]
    t_ptr = np.r_[0, np.cumsum(np.bincount(idx, minlength=num_nodes))].astype(np.int64)
    if fault == "descending_links":
        t_link = np.concatenate([t_link[t_ptr[w]:t_ptr[w + 1]][::-1] for w in range(num_nodes)]) \
            if len(t_link) else t_link
    return t_ptr, t_link.astype(np.int32)


def cn_sum(z, ptr, idx, fault=None):
    return segment_sum(z, ptr, idx, fault)


def cn_sum_grad(grad_out, ptr, idx, num_nodes, fault=None):
    t_ptr, t_link = transpose(ptr, idx, num_nodes, fault)
    return segment_sum(grad_out, t_ptr, t_link, fault)


def values(shape, seed):
    """fp32 uniform in [-1, 1] with |x| >= 2^-20: no subnormal can arise in a sum of them and flush-to-zero cannot
    explain a difference.  The exponents are mixed, so reordering a sum moves its last bit."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, size=shape).astype(np.float32)
    small = np.abs(x) < 2.0 ** -20
    x[small] = np.where(x[small] < 0, -(2.0 ** -20), 2.0 ** -20)
    return x
