"""numpy restatement of the subgraph sketches (kernels in csrc/s3grl_sketch.hip), for
tests/test_sketch_host.py and tests/test_gpu_sketch.py.  Every integer step is exact and every fp64 step is one IEEE
operation in the order §24 fixes, so the GPU's outputs are compared with these to the bit.

    mh, hl = sketches(A, hops, num_perm, hll_p, seed)      # uint32 [hops+1, N, P], uint8 [hops+1, N, m]
    cardinality(rows, hll_p)                                # fp64 E of register rows [..., m]
    match, T, z = raw(mh, hl, links, hll_p)                 # int32 / int64 / int32 [L, hops+1, hops+1]
    I = intersections(match, T, z, num_perm, hll_p)         # fp64 [L, hops+1, hops+1]
    F = features(I, Eu, Ev)                                 # fp64 [L, hops² + 2·hops]
    link_outputs(mh, hl, links, hll_p)                      # all of the above as the device stores them (fp32)
    exact_counts(A, links, hops)                            # the true sets, by breadth-first search

`fault` names one deliberate departure (FAULTS); the tests show that each of them breaks the bit-equality.
"""
import numpy as np
import scipy.sparse as ssp

FAULTS = ("min_without_self", "rank_off_by_one", "match_short", "ie_order")
M32 = np.uint64(0xFFFFFFFF)


def fmix32(h):
    """murmur3's 32-bit finaliser on uint32 values (any shape), arithmetic mod 2^32."""
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def slot_constants(num_slots, seed):
    """c_s = fmix32(seed + s·0x27D4EB2F) for s in 0..num_slots-1."""
    s = np.arange(num_slots, dtype=np.uint64)
    return fmix32((np.uint64(seed) + s * np.uint64(0x27D4EB2F)) & M32)


def hashes(nodes, num_slots, seed):
    """H(v, s) = fmix32(v·0x9E3779B1 + c_s): uint32 [len(nodes), num_slots]."""
    v = np.asarray(nodes, dtype=np.uint64).reshape(-1, 1)
    c = slot_constants(num_slots, seed).astype(np.uint64).reshape(1, -1)
    return fmix32((v * np.uint64(0x9E3779B1) + c) & M32)


def rank(field, hll_p):
    """Leading zeros of the low (32 - p)-bit field + 1; a zero field gives 33 - p."""
    field = np.asarray(field, dtype=np.uint64)
    width = 32 - hll_p
    bits = np.zeros(field.shape, dtype=np.int64)              # bit length of the field
    for b in range(width):
        bits = np.where(field >> np.uint64(b) != 0, b + 1, bits)
    return (width - bits + 1).astype(np.uint8)


def constants(hll_p):
    """(m, R, C, LC): C = α·m²·2^R with α = 0.7213 / (1 + 1.079 / m); LC[z] = m·ln(m / z), LC[0] = inf (unused)."""
    m, R = 1 << hll_p, 33 - hll_p
    alpha = 0.7213 / (1.0 + 1.079 / m)
    C = alpha * m * m * 2.0 ** R
    LC = np.full(m + 1, np.inf)
    LC[1:] = m * np.log(m / np.arange(1, m + 1, dtype=np.float64))
    return m, R, C, LC


def _csr(A):
    A = ssp.csr_matrix(A, copy=True)
    A.sum_duplicates()
    A.eliminate_zeros()
    A.sort_indices()
    return A.indptr.astype(np.int64), A.indices.astype(np.int64)


def _reduce_rows(op, prev, indptr, indices, with_self=True):
    """out[v] = op(prev[v], op over the stored keys w of row v of prev[w])."""
    out = prev.copy()
    deg = np.diff(indptr)
    rows = np.nonzero(deg > 0)[0]
    if len(rows):
        red = op.reduceat(prev[indices], indptr[:-1][rows], axis=0)
        out[rows] = op(out[rows], red) if with_self else red
    return out


def sketches(A, hops=2, num_perm=128, hll_p=8, seed=0, fault=None):
    indptr, indices = _csr(A)
    n, m = len(indptr) - 1, 1 << hll_p
    h = hashes(np.arange(n), num_perm + 1, seed)
    mh = np.empty((hops + 1, n, num_perm), dtype=np.uint32)
    hl = np.zeros((hops + 1, n, m), dtype=np.uint8)
    mh[0] = h[:, :num_perm]
    hh = h[:, num_perm]
    r = rank(hh & np.uint32((1 << (32 - hll_p)) - 1), hll_p)
    hl[0, np.arange(n), hh >> np.uint32(32 - hll_p)] = r + 1 if fault == "rank_off_by_one" else r
    for i in range(1, hops + 1):
        mh[i] = _reduce_rows(np.minimum, mh[i - 1], indptr, indices, with_self=fault != "min_without_self")
        hl[i] = _reduce_rows(np.maximum, hl[i - 1], indptr, indices)
    return mh, hl


def tz(rows, hll_p):
    """(T, z) of register rows [..., m]: T = Σ 2^(R - reg) as int64, z = the zero registers."""
    R = 33 - hll_p
    T = (np.uint64(1) << (np.uint64(R) - rows.astype(np.uint64))).sum(axis=-1, dtype=np.uint64)
    return T.astype(np.int64), (rows == 0).sum(axis=-1).astype(np.int32)


def cardinality_tz(T, z, hll_p):
    m, _, C, LC = constants(hll_p)
    raw = C / T.astype(np.float64)
    return np.where((raw <= 2.5 * m) & (z > 0), LC[z], raw)


def cardinality(rows, hll_p):
    return cardinality_tz(*tz(rows, hll_p), hll_p)


def ball_sizes(hl, hll_p):
    """fp32 [hops+1, N], as SketchGraph.ball_sizes stores them."""
    return cardinality(hl, hll_p).astype(np.float32)


def raw(mh, hl, links, hll_p, fault=None):
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    u, v = links
    K, L = mh.shape[0], links.shape[1]
    slots = mh.shape[2] - 1 if fault == "match_short" else mh.shape[2]
    match = np.zeros((L, K, K), dtype=np.int32)
    T = np.zeros((L, K, K), dtype=np.int64)
    z = np.zeros((L, K, K), dtype=np.int32)
    for i in range(K):
        for j in range(K):
            match[:, i, j] = (mh[i][u, :slots] == mh[j][v, :slots]).sum(axis=1)
            T[:, i, j], z[:, i, j] = tz(np.maximum(hl[i][u], hl[j][v]), hll_p)
    return match, T, z


def intersections(match, T, z, num_perm, hll_p):
    """I_ij = (match_ij · U_ij) / P in fp64: one multiplication, then one division."""
    return (match.astype(np.float64) * cardinality_tz(T, z, hll_p)) / float(num_perm)


def features(I, Eu, Ev, fault=None):
    """I fp64 [L, K, K], Eu / Ev fp64 [L, K] (the endpoints' own ball sizes) -> fp64 [L, hops² + 2·hops] =
    [A_11..A_1k, …, A_kk | Bu_1..Bu_k | Bv_1..Bv_k], every step in §24's order."""
    L, K = I.shape[0], I.shape[1]
    H = K - 1
    zero = np.zeros(L)

    def at(i, j):
        return zero if i < 0 or j < 0 else I[:, i, j]

    def A(i, j):
        if fault == "ie_order":
            return ((at(i, j) - at(i, j - 1)) - at(i - 1, j)) + at(i - 1, j - 1)
        return ((at(i, j) - at(i - 1, j)) - at(i, j - 1)) + at(i - 1, j - 1)

    cols = [A(i, j) for i in range(1, K) for j in range(1, K)]
    for side, E in ((0, Eu), (1, Ev)):
        for i in range(1, K):
            s = np.zeros(L)
            for j in range(0, K):
                s = s + (A(j, i) if side else A(i, j))
            cols.append((E[:, i] - E[:, i - 1]) - s)
    return np.stack(cols, axis=1) if L else np.zeros((0, H * H + 2 * H))


def link_outputs(mh, hl, links, hll_p, fault=None):
    """What SketchGraph.raw / intersections / features return, as numpy: match, T, z and the fp32 outputs."""
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    match, T, z = raw(mh, hl, links, hll_p, fault)
    I = intersections(match, T, z, mh.shape[2], hll_p)
    E = cardinality(hl, hll_p)                                # [K, N]
    F = features(I, E[:, links[0]].T, E[:, links[1]].T, fault)
    return {"match": match, "T": T, "z": z, "intersections": I.astype(np.float32), "features": F.astype(np.float32)}


def exact_counts(A, links, hops, batch=2048):
    """The true sets by breadth-first search over the stored keys: ball B_i(x) = nodes within i steps of x.
    Returns balls_u, balls_v int64 [L, hops+1] (|B_i|), inter int64 [L, hops+1, hops+1] (|B_i(u) ∩ B_j(v)|),
    union likewise, and features fp64 [L, hops² + 2·hops]: A_ij = #{w: d(u,w) = i, d(v,w) = j} for i, j in 1..hops,
    Bu_i = #{w: d(u,w) = i, d(v,w) > hops}, Bv_j = #{w: d(v,w) = j, d(u,w) > hops}."""
    A = ssp.csr_matrix(A)
    S = ssp.csr_matrix((np.ones(A.nnz, dtype=np.float32), A.indices, A.indptr), shape=A.shape)
    n, K = A.shape[0], hops + 1
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    L = links.shape[1]
    out = {"balls_u": np.zeros((L, K), np.int64), "balls_v": np.zeros((L, K), np.int64),
           "inter": np.zeros((L, K, K), np.int64), "union": np.zeros((L, K, K), np.int64),
           "features": np.zeros((L, hops * hops + 2 * hops))}

    def dist(src):
        d = np.full((len(src), n), K, dtype=np.int64)          # K: farther than hops
        ball = np.zeros((len(src), n), dtype=bool)
        ball[np.arange(len(src)), src] = True
        d[ball] = 0
        for i in range(1, K):
            ball = ball | ((ball.astype(np.float32) @ S) > 0)
            d[ball & (d == K)] = i
        return d

    for b0 in range(0, L, batch):
        sl = slice(b0, min(L, b0 + batch))
        du, dv = dist(links[0, sl]), dist(links[1, sl])
        for i in range(K):
            out["balls_u"][sl, i] = (du <= i).sum(1)
            out["balls_v"][sl, i] = (dv <= i).sum(1)
            for j in range(K):
                out["inter"][sl, i, j] = ((du <= i) & (dv <= j)).sum(1)
                out["union"][sl, i, j] = ((du <= i) | (dv <= j)).sum(1)
        cols = [((du == i) & (dv == j)).sum(1) for i in range(1, K) for j in range(1, K)]
        cols += [((du == i) & (dv == K)).sum(1) for i in range(1, K)]
        cols += [((dv == j) & (du == K)).sum(1) for j in range(1, K)]
        out["features"][sl] = np.stack(cols, axis=1)
    return out
