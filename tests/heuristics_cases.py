"""Graphs and link lists that put the CN / AA / PPR kernels (csrc/s3grl_heuristics.hip) on their layout and value
edges, for tests/test_heuristics_host.py (which asserts that the builders deliver what they promise) and
tests/test_gpu_heuristics_shapes.py.  numpy and scipy only; everything is deterministic from fixed seeds.

    comb_graph()        a directed CSR of 700 nodes built row by row: row lengths at the wavefront edges, with the
                        overlap of the two rows of a link chosen, in three value sets
    sink_graph(n, s)    a directed float-weighted graph with sinks (row sum 0, in-edges present), nodes without
                        in-edges and every in-row length 0..9
    star(leaves)        a hub and its leaves, undirected, unit weights
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import scipy.sparse as ssp

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 200)
PATTERNS = ("disjoint", "identical", "first", "last", "below", "above")
# (walked length, searched length) of the pattern cases: the pairs kernel walks the shorter row
PATTERN_PAIRS = ((1, 1), (1, 64), (2, 65), (2, 200), (63, 63), (63, 129), (64, 64), (64, 128), (65, 65), (65, 127),
                 (127, 128), (128, 128), (129, 129), (129, 200), (200, 200))
COMB_NODES = 700
CUT_LENGTHS = (1, 3, 4, 5)
SINK_NS = (1, 15, 16, 17, 49, 1024, 1025, 1041)      # kTile = 16: 1024 is 64 tiles, 1025 is 65; 49: (1/n)·n != 1
COARSE_TOL = 1.0                                     # on sink_graph(1041): columns stop between 1 and 26 iterations
FIXED_KS = (1, 2, 7, 8, 9, 16, 17)                   # around the host's check every 8 iterations, odd and even


def _sample(rng, pool, k):
    return np.sort(rng.choice(np.asarray(pool), k, replace=False))


def _pattern_rows(rng, pattern, lw, ls):
    """(walked row, searched row): sorted column lists of lengths 1 <= lw <= ls whose overlap is `pattern`.  The
    walked row of `first` / `last` also holds the key just outside the searched row's range, and `below` / `above`
    end or begin right next to it."""
    n = COMB_NODES
    S = _sample(rng, range(210, n - 210), ls)           # room for 200 keys on either side
    free = np.setdiff1d(np.arange(n), S)
    if pattern == "identical":
        assert lw == ls
        return S.copy(), S
    if pattern == "disjoint":                            # interleaved with the searched row where that fits
        inside = free[(free > S[0]) & (free < S[-1])]
        return _sample(rng, inside if len(inside) >= lw else free, lw), S
    if pattern in ("first", "last"):
        key, near = (S[0], S[0] - 1) if pattern == "first" else (S[-1], S[-1] + 1)
        W = np.r_[key, near][:lw]
        W = np.r_[W, rng.choice(np.setdiff1d(free, W), lw - len(W), replace=False)]
        return np.sort(W).astype(np.int64), S
    if pattern == "below":
        return np.r_[_sample(rng, range(S[0] - 1), lw - 1), S[0] - 1].astype(np.int64), S
    assert pattern == "above"
    return np.r_[S[-1] + 1, _sample(rng, range(S[-1] + 2, n), lw - 1)].astype(np.int64), S


@lru_cache(maxsize=None)
def comb_graph():
    """A namespace with
      A_int, A_float, A_signed   the same structure [700, 700] with values 1..5, [0.05, 1.55) and ±1 (one in four
                                 negative; a few columns adjusted to sums of exactly 0, exactly 1, 0.5 and -2)
      links [2, L]               every (a, b) of LENGTHS², the pattern cases in both directions, s == d
      cases                      one record per link: (s, d, len s, len d, pattern or None)
      cuts                       {1, 3, 4, 5: positions in `links` of that many links with long rows and common keys}
      columns                    {'zero', 'one', 'half', 'negative': the adjusted columns of A_signed}
    """
    rng = np.random.default_rng(20240611)
    n = COMB_NODES
    rows = []                                            # node id = position

    def add(cols):
        rows.append(np.asarray(cols, dtype=np.int64))
        return len(rows) - 1

    # two generic rows per length: every pair of lengths, overlap as it falls
    generic = {a: (add(_sample(rng, range(n), a)), add(_sample(rng, range(n), a))) for a in LENGTHS}
    cases = []
    for a in LENGTHS:
        for b in LENGTHS:
            cases.append((generic[a][0], generic[b][1], a, b, None))
    for a in LENGTHS:
        cases.append((generic[a][0], generic[a][0], a, a, None))          # s == d
    # the pattern cases, each as (s, d) and (d, s); with equal lengths the kernel walks the smaller id, added first
    for pattern in PATTERNS:
        for lw, ls in PATTERN_PAIRS:
            if pattern == "identical" and lw != ls:
                continue
            W, S = _pattern_rows(rng, pattern, lw, ls)
            w, s = add(W), add(S)
            cases.append((w, s, lw, ls, pattern))
            cases.append((s, w, ls, lw, pattern))
    assert len(rows) <= n
    while len(rows) < n:                                 # the rest: short rows, so that every column has entries
        add(_sample(rng, range(n), int(rng.integers(0, 7))))
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int64)
    indices = np.concatenate(rows).astype(np.int32)
    nnz = len(indices)

    def mat(values):
        return ssp.csr_matrix((np.asarray(values, dtype=np.float64), indices.copy(), indptr.copy()), shape=(n, n))

    A_int = mat(rng.integers(1, 6, nnz))
    A_float = mat(rng.random(nnz) * 1.5 + 0.05)
    signed = rng.choice([-1.0, 1.0, 1.0, 1.0], nnz)      # mostly +1: most column sums stay above 1
    # columns that are common neighbours of some link get exact sums: all entries ±1 but the first, which closes
    # the sum (dyadic values, so the sum is exact in any order)
    links = np.array([[c[0] for c in cases], [c[1] for c in cases]], dtype=np.int64)
    common, common_of = np.zeros(n, dtype=np.int64), []
    for s, d in links.T:
        both = np.intersect1d(rows[s], rows[d])
        common[both] += 1
        common_of.append(len(both))
    count = np.bincount(indices, minlength=n)
    picks = [int(k) for k in np.argsort(-common, kind="stable") if count[k] >= 3][:6]
    picks += [int(k) for k in np.argsort(common, kind="stable") if count[k] >= 3 and common[k] >= 2][:2]   # NaN: rarer
    columns = {}
    for which, target, ks in (("zero", 0.0, picks[0:2]), ("one", 1.0, picks[2:4]), ("half", 0.5, picks[4:6]),
                              ("negative", -2.0, picks[6:8])):
        columns[which] = ks
        for k in ks:
            at = np.nonzero(indices == k)[0]
            signed[at[1:]] = np.where(np.arange(len(at) - 1) % 2 == 0, 1.0, -1.0)
            first = target - signed[at[1:]].sum()
            if first == 0.0:                             # no explicit zero: flip one entry and close again
                signed[at[1]] = -signed[at[1]]
                first = target - signed[at[1:]].sum()
            signed[at[0]] = first
    A_signed = mat(signed)
    long = np.array([i for i, c in enumerate(cases) if min(c[2], c[3]) >= 63 and common_of[i] > 0])
    cuts = {L: long[3 * L:4 * L] for L in CUT_LENGTHS}
    return SimpleNamespace(A_int=A_int, A_float=A_float, A_signed=A_signed, links=links, cases=cases, cuts=cuts,
                           columns=columns, rows=rows)


@lru_cache(maxsize=None)
def sink_graph(n, seed=0):
    """A namespace with A [n, n] (A[i, j]: the arc i -> j, float weights in [0.05, 1.55)), `sinks` (row sum 0),
    `orphans` (no in-edges) and `designated` (nodes whose in-rows have 0, 1, ..., 9 entries; n >= 15).  Built by
    in-rows: about 4 arcs into every node, from nodes that are not sinks.  n = 1 is one node with a self-loop."""
    rng = np.random.default_rng(1000 * n + seed)
    if n == 1:
        A = ssp.csr_matrix(([0.75], ([0], [0])), shape=(1, 1))
        return SimpleNamespace(A=A, sinks=np.zeros(0, np.int64), orphans=np.zeros(0, np.int64),
                               designated=np.zeros(0, np.int64), n=1)
    perm = rng.permutation(n)
    sinks = np.sort(perm[:max(1, n // 10)])
    tails = np.setdiff1d(np.arange(n), sinks)           # nodes that may have out-arcs
    indeg = rng.integers(1, 8, n)
    designated = np.zeros(0, np.int64)
    if n >= 15:
        # in-row lengths 0..9 exactly: 0..8 at nodes with out-arcs, 9 at a sink (r = 0 with in-edges)
        designated = np.r_[rng.choice(tails, 9, replace=False), rng.choice(sinks, 1)]
        indeg[designated] = np.arange(10)
    orphans = rng.choice(np.setdiff1d(np.arange(n), designated), max(1, n // 50), replace=False) if n > 12 else \
        np.zeros(0, np.int64)
    indeg[orphans] = 0
    r, c = [], []
    for j in range(n):
        src = rng.choice(tails, min(int(indeg[j]), len(tails)), replace=False)
        r.append(src)
        c.append(np.full(len(src), j))
    r, c = np.concatenate(r), np.concatenate(c)
    A = ssp.csr_matrix((rng.random(len(r)) * 1.5 + 0.05, (r, c)), shape=(n, n))
    A.sort_indices()
    rs = np.asarray(A.sum(axis=1)).ravel()
    cs = np.diff(A.tocsc().indptr)
    return SimpleNamespace(A=A, sinks=np.nonzero(rs == 0)[0], orphans=np.nonzero(cs == 0)[0],
                           designated=designated, n=n)


def sink_sources(g, ordinary=24, seed=0):
    """Sorted distinct sources of sink_graph `g`: sinks with in-edges, sinks without, nodes without in-edges, the
    designated nodes and some ordinary ones; every node when the graph has at most 64."""
    if g.n <= 64:
        return np.arange(g.n)
    rng = np.random.default_rng(seed + 7)
    rest = np.setdiff1d(np.arange(g.n), np.r_[g.sinks, g.orphans])
    return np.unique(np.r_[g.sinks[:12], g.orphans[:6], g.designated, rng.choice(rest, ordinary, replace=False)])


def links_of(sources, n, per_source=8, seed=0, extra=()):
    """[2, L]: every source with itself, `extra` and `per_source` random destinations, in a shuffled order."""
    rng = np.random.default_rng(seed + 11)
    s, d = [], []
    for u in sources:
        dst = np.r_[u, np.asarray(extra, dtype=np.int64), rng.integers(0, n, per_source)]
        s.append(np.full(len(dst), u))
        d.append(dst)
    L = np.stack([np.concatenate(s), np.concatenate(d)]).astype(np.int64)
    return L[:, rng.permutation(L.shape[1])]


@lru_cache(maxsize=None)
def star(leaves=70000):
    """Node 0 is the hub of `leaves` leaves 1..leaves: undirected, unit weights."""
    n = leaves + 1
    hub, leaf = np.zeros(leaves, dtype=np.int64), np.arange(1, n, dtype=np.int64)
    return ssp.csr_matrix((np.ones(2 * leaves), (np.r_[hub, leaf], np.r_[leaf, hub])), shape=(n, n))
