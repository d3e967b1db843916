"""A numpy restatement of NCNC's completion operators (kernels in s3grl_amd/csrc/s3grl_ncn.hip), as
explicit loops with no torch.  The kernels must equal it to the bit.

    split_lists(A, links, exclude_endpoints)   (counts int64 [3, L], ptr int64 [L+1], idx int32, side int32): per link
                                               S0 = N(u) ∩ N(v), S1 = N(u) \\ N(v), S2 = N(v) \\ N(u), each ascending
    inner_pairs(links, ptr, idx, side)         (inner_at int64, inner_links int32 [2, n]): (w, v) for S1, (u, w) for S2
    segment_wsum(h, ptr, idx, w)               fp32 [R, H]: every term the fp32 product w[j]·h[idx[j], c] rounded once,
                                               the terms added in §26's order (ncn_reference.segment_sum's)
    segment_dot(g, h, ptr, idx)                fp32 [len(idx)]: <g[r(j)], h[idx[j]]> in the fixed slot and tree order
    transposed_weights(w, ptr, idx)            w in the order of ncn_reference.transpose's entries
    wsum_grad_z(g, ptr, idx, w, num_nodes)     the gradient of segment_wsum in h

The order of a dot: slot t of 64 owns the columns c with (c mod 256) // 4 == t; a slot adds its rounded products in
ascending c starting from its first product, a slot without a column holds +0.0; the slots are combined by the halving
tree s = 32, 16, .., 1 (slot t < s becomes slot t + slot t+s); the result is slot 0.

`fault=` gives a named wrong variant; tests/test_ncnc_host.py shows that each leaves byte equality on a case built
for it:
    "contracted"      a term is folded into the sum as one fused multiply-add (fp64 product and sum, rounded once)
    "sequential_dot"  a dot is one plain ascending sum over the columns
    "s2_before_s1"    the sections are stored in the order S0, S2, S1
    "forward_weights" the transposed sum reads the weights in forward order
"""
import numpy as np

import ncn_reference as NR

CHUNK = NR.CHUNK
SLOTS, COL_BLOCK = 64, 256
FAULTS = ("contracted", "sequential_dot", "s2_before_s1", "forward_weights")
values = NR.values


def split_lists(A, links, exclude_endpoints=True, fault=None):
    assert fault in (None,) + FAULTS
    indptr, indices = NR._rows(A)
    u, v = np.asarray(links, dtype=np.int64).reshape(2, -1)
    L = len(u)
    counts = np.zeros((3, L), dtype=np.int64)
    idx, side = [], []
    for l, (a, b) in enumerate(zip(u.tolist(), v.tolist())):
        row_a, row_b = indices[indptr[a]:indptr[a + 1]].tolist(), indices[indptr[b]:indptr[b + 1]].tolist()
        if exclude_endpoints:
            row_a = [k for k in row_a if k != a and k != b]
            row_b = [k for k in row_b if k != a and k != b]
        in_a, in_b = set(row_a), set(row_b)
        sections = [[k for k in row_a if k in in_b], [k for k in row_a if k not in in_b],
                    [k for k in row_b if k not in in_a]]
        counts[:, l] = [len(s) for s in sections]
        for s in ((0, 2, 1) if fault == "s2_before_s1" else (0, 1, 2)):
            idx += sections[s]
            side += [s] * len(sections[s])
    ptr = np.r_[0, np.cumsum(counts.sum(0))].astype(np.int64)
    return counts, ptr, np.asarray(idx, dtype=np.int32), np.asarray(side, dtype=np.int32)


def inner_pairs(links, ptr, idx, side):
    u, v = np.asarray(links, dtype=np.int64).reshape(2, -1)
    at, pairs = [], []
    for l in range(len(ptr) - 1):
        for j in range(int(ptr[l]), int(ptr[l + 1])):
            if side[j] == 1:
                at.append(j)
                pairs.append((idx[j], v[l]))
            elif side[j] == 2:
                at.append(j)
                pairs.append((u[l], idx[j]))
    return np.asarray(at, dtype=np.int64), np.asarray(pairs, dtype=np.int32).reshape(-1, 2).T.copy()


def _chunk(w, rows, fault):
    """the partial of a chunk: its terms w[j]·rows[j] added one after the other, from the first term itself"""
    terms = (w[:, None] * rows).astype(np.float32)         # fp32 x fp32, every product rounded once
    acc = terms[0].copy()
    for j in range(1, len(terms)):
        if fault == "contracted":                          # a fused multiply-add: exact product, one rounding
            acc = (acc.astype(np.float64) + np.float64(w[j]) * rows[j].astype(np.float64)).astype(np.float32)
        else:
            acc = (acc + terms[j]).astype(np.float32)
    return acc


def segment_wsum(h, ptr, idx, w, fault=None):
    assert fault in (None,) + FAULTS
    h, w = np.asarray(h, dtype=np.float32), np.asarray(w, dtype=np.float32)
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    assert len(w) == len(idx)
    R, H = len(ptr) - 1, h.shape[1]
    out = np.zeros((R, H), dtype=np.float32)
    for r in range(R):
        b, e = int(ptr[r]), int(ptr[r + 1])
        if e == b:
            continue                                       # an empty row is +0.0
        partials = [_chunk(w[c:min(c + CHUNK, e)], h[idx[c:min(c + CHUNK, e)]], fault) for c in range(b, e, CHUNK)]
        out[r] = NR._sequential(np.stack(partials))
    return out


def _dots(a, b, fault=None):
    """<a[e], b[e]> of every row e of two [E, H] arrays: the additions are explicit loops in the specified order,
    run for all entries (and all slots) at once"""
    E, H = a.shape
    prod = (a * b).astype(np.float32)                      # fp32 x fp32, rounded once
    if fault == "sequential_dot":
        acc = prod[:, 0].copy()
        for c in range(1, H):
            acc = (acc + prod[:, c]).astype(np.float32)
        return acc
    slots = np.zeros((E, SLOTS), dtype=np.float32)         # a slot without a column holds +0.0
    for c0 in range(0, H, COL_BLOCK):
        for k in range(4):
            cols = np.arange(c0 + k, min(c0 + COL_BLOCK, H), 4)       # column c0 + 4 t + k of slot t, for t < len(cols)
            t = len(cols)
            if t == 0:
                continue
            if c0 == 0 and k == 0:
                slots[:, :t] = prod[:, cols]               # the first product starts the slot's sum
            else:
                slots[:, :t] = (slots[:, :t] + prod[:, cols]).astype(np.float32)
    s = SLOTS // 2
    while s >= 1:
        slots[:, :s] = (slots[:, :s] + slots[:, s:2 * s]).astype(np.float32)
        s //= 2
    return slots[:, 0].copy()


def segment_dot(g, h, ptr, idx, fault=None, block=32768):
    assert fault in (None,) + FAULTS
    g, h = np.asarray(g, dtype=np.float32), np.asarray(h, dtype=np.float32)
    ptr, idx = np.asarray(ptr, dtype=np.int64), np.asarray(idx, dtype=np.int64)
    owner = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))      # r(j): the list that holds entry j
    out = np.zeros(len(idx), dtype=np.float32)
    for e0 in range(0, len(idx), block):
        out[e0:e0 + block] = _dots(g[owner[e0:e0 + block]], h[idx[e0:e0 + block]], fault)
    return out


def transposed_weights(w, ptr, idx, fault=None):
    """the weight of every entry of ncn_reference.transpose(ptr, idx, .), in its order"""
    assert fault in (None,) + FAULTS
    w = np.asarray(w, dtype=np.float32)
    if fault == "forward_weights":
        return w.copy()
    return w[np.argsort(np.asarray(idx, dtype=np.int64), kind="stable")]


def wsum_grad_z(g, ptr, idx, w, num_nodes, fault=None):
    t_ptr, t_link = NR.transpose(ptr, idx, num_nodes)
    return segment_wsum(g, t_ptr, t_link, transposed_weights(w, ptr, idx, fault), fault)


def weights(n, seed):
    """fp32 weights with both signs and mixed exponents, |x| >= 2^-20, with exact 0.0, -0.0 and 1.0 among them"""
    w = values((n,), seed)
    if n >= 3:
        w[n // 3], w[n // 2], w[-1] = 0.0, -0.0, 1.0
    return w
