"""Case builders for the link-recommendation kernels (test infrastructure; numpy and scipy only, no GPU): graphs whose
rows sit on the edges of candidates_kernel's two row walks, source lists that make a resident workgroup of the HBM
flavour take one source after another, and fp32 scores built from bit patterns for segment_topk_kernel's radix select
and tie sweep.  tests/test_recommend_host.py asserts what each builder promises."""
import numpy as np
import scipy.sparse as ssp

import recommend_reference as ref

HUB_SIZES = (4096, 4097, 131073, 524289)
HUB_ROWS = {"hub15": 15, "hub16": 16, "hub17": 17, "hub63": 63, "hub64": 64, "hub65": 65, "hub128": 128,
            "hub129": 129, "hub_big": 1029}
CHORD_EVERY, CHORD = 64, 1234            # the chorded ring of tests/test_gpu_recommend.py
LARGE, TINY, EMPTY = 0, 1, 2             # the kinds of stride_sources


# ---- graphs ------------------------------------------------------------------------------------------------------------
def hub_names(ids):
    return [name for name in ids if name.startswith("hub")]


def isolated_names(ids):
    return [name for name in ids if name.startswith("iso")]


def hub_graph(n):
    """(A, ids, rows): the chorded ring of n nodes with planted hubs.  `ids` names nodes, `rows` gives the final row
    length of each named node.

    - hub15 ... hub129, hub_big: rows of exactly 15, 16, 17, 63, 64, 65, 128, 129 and 1 029 entries (ring, chord and
      planted edges together).  hub_big is node 0, hub128 is node n - 1, hub17 and hub65 share a 32-node bitmap word,
      hub64 and hub129 sit in different words of one 64-word chunk, the other three lie in the upper half of the ids.
      The planted neighbours of a hub step evenly down the whole id range from n - 2.
    - x is adjacent to every hub and to s, s to x alone: the level-2 frontier of s is the hub set.
    - iso0, iso1 (adjacent ids) and iso2 have empty rows.
    """
    if n not in HUB_SIZES:
        raise ValueError(f"hub_graph: n must be one of {HUB_SIZES}, got {n}")
    ids = {"s": 501, "x": 500, "iso0": 40, "iso1": 41, "iso2": n // 3,
           "hub_big": 0, "hub128": n - 1, "hub17": 1000, "hub65": 1003, "hub64": 2100, "hub129": 2200,
           "hub15": n // 2 + 7, "hub16": (3 * n) // 4 + 1, "hub63": n - 200}
    assert len(set(ids.values())) == len(ids)
    special = set(ids.values())
    carved = np.array([ids[name] for name in ["s", "x"] + isolated_names(ids)])
    i = np.arange(n, dtype=np.int64)
    c = i[::CHORD_EVERY]
    base = np.concatenate([np.stack([i, (i + 1) % n], 1), np.stack([c, (c + CHORD) % n], 1)])
    base = base[~(np.isin(base[:, 0], carved) | np.isin(base[:, 1], carved))]
    nbrs = {name: set() for name in HUB_ROWS}
    node_hub = {ids[name]: name for name in HUB_ROWS}
    for a, b in base[np.isin(base[:, 0], list(node_hub)) | np.isin(base[:, 1], list(node_hub))].tolist():
        if a in node_hub:
            nbrs[node_hub[a]].add(b)
        if b in node_hub:
            nbrs[node_hub[b]].add(a)
    planted = [(ids["s"], ids["x"])]
    for j, (name, want) in enumerate(HUB_ROWS.items()):
        h = ids[name]
        planted.append((ids["x"], h))
        have = nbrs[name] | {ids["x"]}
        m = want - len(have)
        assert m > 0
        for t in range(m):
            v = (n - 2 - 3 * j - (t * (n - 3)) // m) % n
            while v in special or v in have:
                v = (v - 1) % n
            have.add(v)
            planted.append((h, v))
    A = ref.csr_of(n, np.concatenate([base, np.asarray(planted, dtype=np.int64)]))
    rows = {name: int(A.indptr[v + 1] - A.indptr[v]) for name, v in ids.items()}
    return A, ids, rows


def star(n):
    """Node 0 joined to each of 1 ... n - 1."""
    v = np.arange(1, n, dtype=np.int64)
    return ref.csr_of(n, np.stack([np.zeros_like(v), v], 1))


def path(n, start=0, num_nodes=None):
    """The path start - start + 1 - ... - start + n - 1 in a graph of num_nodes (default start + n) nodes."""
    v = np.arange(start, start + n - 1, dtype=np.int64)
    return ref.csr_of(start + n if num_nodes is None else num_nodes, np.stack([v, v + 1], 1))


def two_paths(a, b):
    """Two disjoint paths: nodes 0 ... a - 1 and a ... a + b - 1."""
    return (path(a, 0, a + b) + path(b, a, a + b)).tocsr()


def quiet_nodes(A, ids, hops):
    """Ring nodes (ascending) more than hops + 1 steps away, on the graph, from every endpoint of a planted edge and
    from every carved node: the ball of radius `hops` around one is ring and chord edges alone."""
    n = A.shape[0]
    seed = np.zeros(n, dtype=bool)
    for name, v in ids.items():
        seed[v] = True
        if name.startswith("hub"):
            seed[A.indices[A.indptr[v]:A.indptr[v + 1]]] = True
    seed[[(ids[name] + d) % n for name in ["s", "x"] + isolated_names(ids) for d in (-1, 1)]] = True
    B = ssp.csr_matrix((np.ones(A.nnz, dtype=np.int32), A.indices, A.indptr), shape=A.shape)
    reach = seed.copy()
    for _ in range(hops + 1):
        reach |= (B @ reach.astype(np.int32)) > 0
    return np.nonzero(~reach)[0]


def stride_sources(graph_info, resident, rounds, hops=3):
    """(sources int64 [rounds * resident + 5], kinds): position p is taken by resident workgroup p % resident in its
    turn p // resident, and the kinds a workgroup meets in turn rotate LARGE (a hub or s) -> TINY (a quiet ring node)
    -> EMPTY (an isolated node)."""
    A, ids, _ = graph_info
    large = [ids[name] for name in hub_names(ids)] + [ids["s"]]
    quiet = quiet_nodes(A, ids, hops)
    tiny = quiet[np.linspace(0, len(quiet) - 1, 61).astype(np.int64)].tolist()
    empty = [ids[name] for name in isolated_names(ids)]
    p = np.arange(rounds * resident + 5)
    kinds = (p % resident + p // resident) % 3
    pools = {LARGE: large, TINY: tiny, EMPTY: empty}
    sources = np.array([pools[kind][q % len(pools[kind])] for q, kind in zip(p.tolist(), kinds.tolist())],
                       dtype=np.int64)
    return sources, kinds


def candidates_tiled(A, sources, hops, exclude=None):
    """ref.candidates for a long list with many repeats: one walk per distinct source, the segments tiled."""
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    distinct, inverse = np.unique(sources, return_inverse=True)
    ptr, cand = ref.candidates(A, distinct, hops, exclude)
    segs = [cand[ptr[j]:ptr[j + 1]] for j in range(len(distinct))]
    picked = [segs[j] for j in inverse.tolist()]
    seg_ptr = np.concatenate([[0], np.cumsum([len(x) for x in picked])]).astype(np.int64)
    return seg_ptr, (np.concatenate(picked) if picked else np.zeros(0)).astype(np.int32)


# ---- scores, from bit patterns -------------------------------------------------------------------------------------------
def order_key(scores):
    """order_key of csrc/s3grl_recommend.hip in numpy: NaN -> 0, -0.0 -> +0.0, then the sign flip."""
    u = np.asarray(scores, dtype=np.float32).view(np.uint32).copy()
    nan = (u & 0x7fffffff) > 0x7f800000
    u[u == 0x80000000] = 0
    key = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    key[nan] = 0
    return key


def digit_scores(n, digit, rng, negative=False, cuts=()):
    """n scores whose keys agree in every bit above 8-bit digit `digit` (0 = the least significant byte) and vary in
    that digit and below, drawn from about n / 4 distinct values, all positive or all negative.  For every k in
    `cuts` with k < n the k-th and the (k + 1)-th best score are equal: the cut falls inside a tie group."""
    low = 8 * (digit + 1)
    sign = 0x80000000 if negative else 0
    if low == 32:                                   # the top byte varies: any finite magnitude
        values = rng.integers(0, 0x7f800000, max(2, n // 4), dtype=np.uint32)
    else:
        values = (0x3f800000 >> low << low) | rng.integers(0, 1 << low, max(2, n // 4), dtype=np.uint32)
    bits = (values | sign).astype(np.uint32)[rng.integers(0, len(values), n)]
    for k in sorted(cuts):
        if k < n:
            order = np.argsort(~order_key(bits.view(np.float32)), kind="stable")      # best first
            bits[order[k]] = bits[order[k - 1]]
    return bits.view(np.float32)


def any_finite(n, rng):
    """Uniform over every non-NaN bit pattern, with both zeros, both infinities and the smallest and largest
    denormals of both signs planted (twice each where n allows)."""
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    nan = (bits & 0x7fffffff) > 0x7f800000
    bits[nan] &= 0xff800000                         # a NaN becomes the infinity of its sign
    plant = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001, 0x007fffff,
                      0x807fffff] * 2, dtype=np.uint32)[:n // 2]
    bits[rng.choice(n, len(plant), replace=False)] = plant
    return bits.view(np.float32)


def nan_heavy(n, keep, rng):
    """Exactly `keep` non-NaN scores (quantised normals) at random positions, NaNs of random payload and sign
    elsewhere."""
    bits = (0x7f800000 | rng.integers(1, 1 << 23, n, dtype=np.uint32) |
            (rng.integers(0, 2, n, dtype=np.uint32) << 31)).astype(np.uint32)
    s = bits.view(np.float32).copy()
    where = rng.choice(n, keep, replace=False)
    s[where] = (np.round(rng.standard_normal(keep) * 4) / 4).astype(np.float32)
    return s


def ties_at(n, k, r, where, extra=3):
    """(scores, tie positions ascending): k - r scores of 2.0 (above the cut), r + extra of 1.0 (the ties: the cut
    takes the r of lowest position), 0.0 elsewhere.
      "head": the ties are positions 0 ... r + extra - 1;   "tail": the last r + extra positions;
      "spread": dealt round the 256-position chunks, one per chunk while there are no more ties than chunks."""
    t = r + extra
    if where == "head":
        pos = np.arange(t)
    elif where == "tail":
        pos = np.arange(n - t, n)
    else:
        assert where == "spread"
        chunks = -(-n // 256)
        j = np.arange(t)
        pos = 256 * (j % chunks) + (37 * (j % chunks) + 3 * (j // chunks)) % 100
    pos = np.sort(pos)
    assert len(np.unique(pos)) == t and pos[-1] < n
    s = np.zeros(n, dtype=np.float32)
    free = np.setdiff1d(np.arange(n), pos)
    s[free[np.linspace(0, len(free) - 1, k - r).astype(np.int64)]] = 2.0
    s[pos] = 1.0
    assert int((s == 2.0).sum()) == k - r
    return s, pos


def constant(n, what):
    return np.full(n, {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[what], dtype=np.float32)


# the radix-select cases of tests/test_gpu_recommend_shapes.py: three segments beyond the in-LDS sort (2 048 entries),
# short ones between them, every k in one list so that one score array serves them all
SELECT_LENGTHS = (2049, 1, 4097, 2, 3, 10000, 5, 2048)
SELECT_KS = (1, 2, 3, 100, 1000, 1023, 1024)


def select_case(kind, seed):
    """The scores of SELECT_LENGTHS laid end to end: kind ("digit", d, negative) -> digit_scores per segment with a
    tie across every cut of SELECT_KS; "any_finite" -> any_finite per segment."""
    rng = np.random.default_rng(seed)
    if kind == "any_finite":
        return np.concatenate([any_finite(n, rng) for n in SELECT_LENGTHS])
    _, digit, negative = kind
    return np.concatenate([digit_scores(n, digit, rng, negative, cuts=SELECT_KS) for n in SELECT_LENGTHS])
