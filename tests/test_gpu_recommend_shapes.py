"""Link recommendation on the MI355X, second pass: the paths of candidates_kernel and segment_topk_kernel that
tests/test_gpu_recommend.py does not reach, on the cases of tests/recommend_cases.py (whose promises
tests/test_recommend_host.py asserts).  Long rows under every workgroup size and in the HBM flavour, a resident
workgroup taking several sources, hops up to 8, exclusion keys beyond 2^32, the radix select decided in a chosen digit,
the NaN class as the threshold, ties placed for the sweep's earliest and latest stop, seg_ptr with slack, output views,
empty lists and large launches.  Every comparison with tests/recommend_reference.py is exact: integers equal, fp32 bit
for bit."""
import numpy as np
import pytest
import torch

import recommend_cases as cases
import recommend_reference as ref
from conftest import load_extract

pytestmark = pytest.mark.gpu

LDS_SORT = 2048          # kTopSort of csrc/s3grl_recommend.hip: longer segments go through the radix select
SERIAL_ROW = 16          # kSerialRow: longer rows are walked by the whole wavefront
SCAN_TILE = 1024         # kScanTile of csrc/s3grl_structure.hip: the int32 -> int64 scan that makes seg_ptr
TOP_T = 256              # kTopT: positions per barrier of the tie sweep
MAX_K = 1024             # kTopMaxK


@pytest.fixture(scope="module")
def eng():
    from s3grl_amd.engine import default_engine

    return default_engine("cuda:0")


@pytest.fixture(scope="module")
def hub(eng):
    """n -> (A, ids, rows, graph on the device), built once per size."""
    made = {}

    def get(n):
        if n not in made:
            A, ids, rows = cases.hub_graph(n)
            made[n] = (A, ids, rows, eng.graph(A))
        return made[n]

    yield get
    for entry in made.values():
        entry[3].close()


def _compare(g, A, sources, hops, exclude=None, reference=ref.candidates):
    from s3grl_amd import recommend as R

    seg_ptr, cand = R.candidates(g, sources, hops, exclude)
    assert seg_ptr.dtype == torch.int64 and cand.dtype == torch.int32 and seg_ptr.is_cuda and cand.is_cuda
    want_ptr, want = reference(A, sources, hops, exclude)
    assert np.array_equal(seg_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(cand.cpu().numpy(), want)
    return want_ptr, want


def _fresh(eng, A, sources, hops, exclude=None):
    g = eng.graph(A)
    try:
        return _compare(g, A, sources, hops, exclude)
    finally:
        g.close()


def _row(A, v):
    return A.indices[A.indptr[v]:A.indptr[v + 1]]


# ---- candidates: long rows under every instantiation -------------------------------------------------------------------
def _hub_sources(A, ids):
    n = A.shape[0]
    hubs = [ids[h] for h in cases.hub_names(ids)]
    special = set(ids.values())
    nbrs = [int(next(v for v in _row(A, h)[len(_row(A, h)) // 2:] if v not in special)) for h in hubs]
    return [ids["s"], ids["x"]] + hubs + nbrs + [ids[name] for name in cases.isolated_names(ids)] + [0, n - 1]


# 4 096: 64 threads, two chunks for the one wavefront; 4 097: 256 threads, the last chunk one live lane that owns the
# hub n - 1; 131 073: 1 024 threads; 524 289: the HBM flavour.  hops 5 and 8 at 4 097: balls that fill most words.
@pytest.mark.parametrize("n,hops", [(4096, 2), (4096, 3), (4097, 2), (4097, 3), (4097, 5), (4097, 8), (131073, 2),
                                    (131073, 3), (524289, 2), (524289, 3)])
def test_hub_rows_under_every_workgroup_size(hub, n, hops):
    from s3grl_amd import recommend as R

    A, ids, rows, g = hub(n)
    lay = R.layout(n)
    assert (lay["bitmap"], lay["threads"]) == {4096: ("lds", 64), 4097: ("lds", 256), 131073: ("lds", 1024),
                                               524289: ("hbm", 1024)}[n]
    assert rows["hub16"] == SERIAL_ROW and rows["hub17"] == SERIAL_ROW + 1 and rows["hub_big"] > 1024
    sources = _hub_sources(A, ids)
    ptr, cand = _compare(g, A, sources, hops)
    size = dict(zip(sources, np.diff(ptr).tolist()))
    assert all(size[ids[name]] == 0 for name in cases.isolated_names(ids))
    assert size[ids["x"]] > sum(cases.HUB_ROWS.values()) // 2           # x at 2 hops: the rows of all hubs
    if hops >= 3:                                                       # s at 3 hops: the hubs and their rows
        assert size[ids["s"]] > sum(cases.HUB_ROWS.values()) // 2
        assert set(ids[h] for h in cases.hub_names(ids)) <= set(cand[ptr[0]:ptr[1]].tolist())
    if hops == 8:
        assert size[ids["s"]] > n // 2


@pytest.mark.parametrize("n", [4097, 131073])
def test_star_leaf_segments_hold_every_other_leaf(eng, n):
    sources = [0, 1, n - 1, n // 2, n // 3]
    ptr, cand = _fresh(eng, cases.star(n), sources, 2)
    assert np.diff(ptr).tolist() == [0] + [n - 2] * 4
    assert cand[ptr[1]:ptr[2]].tolist() == list(range(2, n)) and cand[ptr[2]:ptr[3]].tolist() == list(range(1, n - 1))


@pytest.mark.parametrize("hops", [2, 3, 4, 5, 6, 7, 8])
def test_path_of_twelve(eng, hops):
    ptr, cand = _fresh(eng, cases.path(12), [0, 6, 1, 11], hops)
    assert cand[ptr[0]:ptr[1]].tolist() == list(range(2, hops + 1))                 # from an end
    assert cand[ptr[1]:ptr[2]].tolist() == [v for v in range(12) if 2 <= abs(v - 6) <= hops]   # the walk ends early
    assert cand[ptr[2]:ptr[3]].tolist() == list(range(3, min(hops + 2, 12)))
    assert cand[ptr[3]:ptr[4]].tolist() == list(range(11 - hops, 10))


def test_two_disjoint_paths_do_not_mix(eng):
    sources = [0, 11, 12, 18, 5, 15]
    ptr, cand = _fresh(eng, cases.two_paths(12, 7), sources, 8)
    for i, u in enumerate(sources):
        seg = cand[ptr[i]:ptr[i + 1]]
        assert len(seg) and np.all((seg < 12) == (u < 12))


# ---- candidates: the HBM flavour's resident workgroups take several sources ------------------------------------------
@pytest.mark.parametrize("with_exclude", [False, True])
def test_hbm_workgroups_reuse_their_slices(hub, with_exclude):
    from s3grl_amd import recommend as R

    n, hops = 524289, 3
    A, ids, rows, g = hub(n)
    resident = R.layout(n)["resident_workgroups"]
    sources, kinds = cases.stride_sources((A, ids, rows), resident, 2, hops)
    assert resident > 0 and len(sources) == 2 * resident + 5          # some workgroups take three sources
    exclude = None
    if with_exclude:
        plain_ptr, plain = cases.candidates_tiled(A, sources, hops)
        big, tiny = int(np.nonzero(kinds == cases.LARGE)[0][0]), int(np.nonzero(kinds == cases.TINY)[0][0])
        third = plain[plain_ptr[big]:plain_ptr[big + 1]][::3]
        exclude = np.array([[sources[big]] * len(third) + [int(plain[plain_ptr[tiny]])],
                            third.tolist() + [sources[tiny]]], dtype=np.int64)
    ptr, cand = _compare(g, A, sources, hops, exclude, reference=cases.candidates_tiled)
    size = np.diff(ptr)
    assert np.all(size[kinds == cases.EMPTY] == 0) and size[kinds == cases.LARGE].min() > 1000
    again = R.candidates(g, sources, hops, exclude)
    assert np.array_equal(again[0].cpu().numpy(), ptr) and np.array_equal(again[1].cpu().numpy(), cand)


def test_hbm_bad_source_inside_a_stride_is_reported(eng, hub):
    from s3grl_amd import recommend as R

    n, hops = 524289, 3
    A, ids, rows, g = hub(n)
    resident = R.layout(n)["resident_workgroups"]
    sources, _ = cases.stride_sources((A, ids, rows), resident, 2, hops)
    bad = sources.copy()
    bad[resident + 3] = n                                             # the second source of workgroup 3
    with pytest.raises(ValueError, match="source"):
        R._count(g, torch.as_tensor(bad, dtype=torch.int32).to(eng.device), hops, None)
    _compare(g, A, sources, hops, reference=cases.candidates_tiled)   # and the graph object still serves


def test_more_sources_than_the_scan_tile(eng):
    z = load_extract("rand300")
    A = ref.csr_of(300, z["edges"])
    sources = np.concatenate([np.tile(np.arange(300), 4), [7, 7, 299, 0, 7]])
    assert len(sources) > SCAN_TILE
    g = eng.graph(A)
    try:
        ptr, _ = _compare(g, A, sources, 2, reference=cases.candidates_tiled)
    finally:
        g.close()
    assert np.array_equal(np.diff(ptr)[:300], np.diff(ptr)[900:1200])


# ---- candidates: exclusion keys beyond 2^32 ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [131073, 524289])
def test_exclusion_keys_beyond_32_bits(eng, hub, n):
    from s3grl_amd import recommend as R

    A, ids, _, g = hub(n)
    lim = -(-(1 << 32) // n)                                          # min(u, v) >= lim: the key is 2^32 or more
    quiet = cases.quiet_nodes(A, ids, 2)
    q_hi, q_mid = int(quiet[-1]), int(quiet[len(quiet) // 2])
    top, first = ids["hub128"], ids["hub_big"]
    assert lim + 10 < q_mid < q_hi - 10 and first == 0 and top == n - 1
    sources = [first, q_mid, q_hi, top, ids["hub16"], q_mid]
    plain_ptr, plain = ref.candidates(A, sources, 2)
    seg = [plain[plain_ptr[i]:plain_ptr[i + 1]] for i in range(len(sources))]
    high = seg[3][(seg[3] >= lim) & (seg[3] < q_hi - 10)][::2]        # every second such candidate of node n - 1
    assert len(high) > 20 and len(seg[1]) >= 2 and seg[1].min() >= lim
    pairs = [(q_mid, int(seg[1][0]))] + [(int(v), q_mid) for v in seg[1][1:]]      # every candidate of q_mid
    pairs += [(int(v), top) for v in high] + [(q_mid, q_mid)]                       # ... and the self pair
    keys = sorted(min(a, b) * n + max(a, b) for a, b in pairs)
    assert keys[0] >= 1 << 32 and len({key & 0xffffffff for key in keys}) == len(keys)
    probes = lambda i: [min(sources[i], int(v)) * n + max(sources[i], int(v)) for v in seg[i]]   # noqa: E731
    assert max(probes(0)) < keys[0] and min(probes(2)) > keys[-1]     # every probe below the list; every probe above
    exclude = np.array(pairs, dtype=np.int64).T
    ptr, cand = _compare(g, A, sources, 2, exclude)
    assert np.diff(ptr).tolist() == [len(seg[0]), 0, len(seg[2]), len(seg[3]) - len(high),
                                     np.diff(ptr)[4], 0]              # q_mid emptied, its neighbours as they were
    assert np.array_equal(cand[ptr[2]:ptr[3]], seg[2]) and np.array_equal(cand[:ptr[1]], seg[0])
    # the same list as an int32 tensor on the host and as an int64 tensor on the device
    for form in (torch.as_tensor(exclude, dtype=torch.int32), torch.as_tensor(exclude).to(eng.device)):
        got = R.candidates(g, sources, 2, form)
        assert np.array_equal(got[0].cpu().numpy(), ptr) and np.array_equal(got[1].cpu().numpy(), cand)
    # a list of one key: probes below it (node 0), above it (q_hi), and the key itself
    one = np.array([[top], [int(high[len(high) // 2])]], dtype=np.int64)
    ptr1, cand1 = _compare(g, A, [first, top, q_hi], 2, one)
    assert np.diff(ptr1).tolist() == [len(seg[0]), len(seg[3]) - 1, len(seg[2])] and int(one[1, 0]) not in \
        cand1[ptr1[1]:ptr1[2]]


# ---- empty lists -------------------------------------------------------------------------------------------------------
def test_empty_source_list(eng, hub):
    from s3grl_amd import recommend as R

    _, _, _, g = hub(4096)
    for empty in ([], np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int32, device=eng.device)):
        seg_ptr, cand = R.candidates(g, empty, 2)
        assert seg_ptr.tolist() == [0] and seg_ptr.dtype == torch.int64 and tuple(cand.shape) == (0,)
        assert cand.dtype == torch.int32
    top = R.segment_topk(torch.zeros(0, device=eng.device), torch.zeros(1, dtype=torch.int64, device=eng.device),
                         torch.zeros(0, dtype=torch.int32, device=eng.device), 7, engine=eng)
    assert tuple(top.nodes.shape) == (0, 7) and tuple(top.scores.shape) == (0, 7) and tuple(top.count.shape) == (0,)

    def scorer(pairs):
        raise AssertionError("no pairs: the scorer must not run")

    top = R.recommend(g, [], scorer, k=3)
    assert tuple(top.nodes.shape) == (0, 3) and tuple(top.scores.shape) == (0, 3) and tuple(top.count.shape) == (0,)
    assert top.nodes.dtype == torch.int32 and top.scores.dtype == torch.float32 and top.count.dtype == torch.int32


# ---- segment top-K -----------------------------------------------------------------------------------------------------
def _check_topk(eng, scores, seg_ptr, k, cand=None):
    """segment_topk against the restatement, exactly; seg_ptr may leave a head and a tail of scores / cand unused."""
    from s3grl_amd import recommend as R

    scores = np.asarray(scores, dtype=np.float32)
    seg_ptr = np.asarray(seg_ptr, dtype=np.int64)
    if cand is None:
        cand = np.random.default_rng(5).integers(0, 1 << 30, len(scores)).astype(np.int32)
    s_dev = torch.as_tensor(scores).to(eng.device)
    top = R.segment_topk(s_dev, torch.as_tensor(seg_ptr).to(eng.device), torch.as_tensor(cand).to(eng.device), k,
                         engine=eng)
    read_back = s_dev.cpu().numpy()
    assert np.array_equal(read_back.view(np.int32), scores.view(np.int32))        # NaN payloads survive the copy
    nodes, vals, count = ref.segment_topk(read_back, seg_ptr, cand, k)
    assert top.nodes.dtype == torch.int32 and top.scores.dtype == torch.float32 and top.count.dtype == torch.int32
    assert np.array_equal(top.count.cpu().numpy(), count)
    assert np.array_equal(count, np.minimum(k, np.diff(seg_ptr)))
    assert np.array_equal(top.nodes.cpu().numpy(), nodes)
    assert np.array_equal(top.scores.cpu().numpy().view(np.int32), vals.view(np.int32))      # bit for bit
    return nodes, vals, count


def _ptr_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


SELECT_KINDS = [("digit", d, neg) for d in (0, 1, 2, 3) for neg in (False, True)] + ["any_finite"]


@pytest.mark.parametrize("k", cases.SELECT_KS)
@pytest.mark.parametrize("kind", SELECT_KINDS, ids=lambda kind: kind if isinstance(kind, str) else
                         f"digit{kind[1]}{'neg' if kind[2] else 'pos'}")
def test_radix_select_decided_in_a_chosen_digit(eng, kind, k):
    assert sum(n > LDS_SORT for n in cases.SELECT_LENGTHS) == 3 and LDS_SORT in cases.SELECT_LENGTHS
    assert MAX_K in cases.SELECT_KS and MAX_K - 1 in cases.SELECT_KS
    _check_topk(eng, cases.select_case(kind, seed=4), _ptr_of(cases.SELECT_LENGTHS), k)


@pytest.mark.parametrize("k", [10, 1000])
def test_nan_class_as_the_threshold(eng, k):
    rng = np.random.default_rng(k)
    n = 3000
    keeps = [0, 1, k - 5, k - 1, k, k + 1]
    segs = [cases.nan_heavy(n, keep, rng) for keep in keeps]
    low = cases.nan_heavy(n, k - 3, rng)
    low[~np.isnan(low)] = -np.inf                                      # -inf everywhere except the NaNs
    segs.append(low)
    segs += [cases.constant(m, what) for m in (LDS_SORT + 1, 5000) for what in ("+inf", "-inf", "nan")]
    lengths = [len(x) for x in segs]
    ptr = _ptr_of(lengths)
    position = np.concatenate([np.arange(m, dtype=np.int32) for m in lengths])     # cand = position in the segment
    nodes, vals, count = _check_topk(eng, np.concatenate(segs), ptr, k, cand=position)
    assert count.tolist() == [k] * len(segs)
    for i, keep in enumerate(keeps + [k - 3]):
        got_nan = np.isnan(vals[i])
        assert int(got_nan.sum()) == max(0, k - keep) and not got_nan[:min(keep, k)].any()
        if keep < k:                                                   # the NaNs taken are those of lowest position
            assert np.array_equal(nodes[i][keep:], np.nonzero(np.isnan(segs[i]))[0][:k - keep])
    for i in range(len(keeps) + 1, len(segs)):                         # constants: the first k positions
        assert nodes[i].tolist() == list(range(k))


@pytest.mark.parametrize("k", [64, 1000])
@pytest.mark.parametrize("where", ["head", "tail", "spread"])
def test_tie_sweep_with_placed_ties(eng, where, k):
    n = 6000
    assert n > LDS_SORT and n % TOP_T != 0
    made = [cases.ties_at(n, k, r, where) for r in (1, 7, k)]
    position = np.tile(np.arange(n, dtype=np.int32), len(made))
    nodes, vals, _ = _check_topk(eng, np.concatenate([s for s, _ in made]), _ptr_of([n] * len(made)), k, cand=position)
    for i, r in enumerate((1, 7, k)):
        assert np.array_equal(nodes[i][k - r:], made[i][1][:r]) and np.all(vals[i][k - r:] == 1.0)
        assert np.all(vals[i][:k - r] == 2.0)


@pytest.mark.parametrize("k", [10, 1024])
def test_seg_ptr_with_slack_at_both_ends(eng, k):
    rng = np.random.default_rng(k)
    lengths = [3, LDS_SORT + 1, 0, 300, 5000]
    body = (np.round(rng.standard_normal(sum(lengths)) * 4) / 4).astype(np.float32)
    head, tail = [np.inf, np.nan, np.inf, np.nan, np.inf], [np.nan, np.inf] * 3 + [np.inf]
    scores = np.concatenate([head, body, tail]).astype(np.float32)
    sentinel = -7777
    cand = np.concatenate([[sentinel] * 5, rng.integers(0, 1 << 30, len(body)), [sentinel] * 7]).astype(np.int32)
    seg_ptr = 5 + _ptr_of(lengths)
    assert seg_ptr[0] == 5 and seg_ptr[-1] == len(scores) - 7
    nodes, vals, _ = _check_topk(eng, scores, seg_ptr, k, cand=cand)
    assert sentinel not in nodes and not np.isnan(vals).any() and not np.isposinf(vals).any()


def test_output_rows_through_views(eng):
    from s3grl_amd import recommend as R

    k, lengths = 5, [0, 3, LDS_SORT + 7, 5, 64]
    S = len(lengths)
    rng = np.random.default_rng(13)
    scores = (np.round(rng.standard_normal(sum(lengths)) * 4) / 4).astype(np.float32)
    cand = rng.integers(0, 1 << 30, len(scores)).astype(np.int32)
    seg_ptr = _ptr_of(lengths)
    dev = eng.device
    nodes = torch.full((S + 2, k), -99, dtype=torch.int32, device=dev)
    vals = torch.full((S + 2, k), 123.5, dtype=torch.float32, device=dev)
    count = torch.full((S + 2,), -99, dtype=torch.int32, device=dev)
    R._topk_into(eng, torch.as_tensor(scores).to(dev), torch.as_tensor(seg_ptr).to(dev), torch.as_tensor(cand).to(dev),
                 k, nodes[1:S + 1], vals[1:S + 1], count[1:S + 1])
    want_nodes, want_vals, want_count = ref.segment_topk(scores, seg_ptr, cand, k)
    nodes, vals, count = nodes.cpu().numpy(), vals.cpu().numpy(), count.cpu().numpy()
    for row in (0, S + 1):                                             # the neighbouring rows are left alone
        assert np.all(nodes[row] == -99) and np.all(vals[row] == 123.5) and count[row] == -99
    assert np.array_equal(nodes[1:S + 1], want_nodes) and np.array_equal(count[1:S + 1], want_count)
    assert np.array_equal(vals[1:S + 1].view(np.int32), want_vals.view(np.int32))
    for i in range(S):
        assert np.all(nodes[1 + i, count[1 + i]:] == -1) and np.all(np.isneginf(vals[1 + i, count[1 + i]:]))


def test_seventy_thousand_short_segments(eng):
    S, k = 70000, 3
    lengths = np.arange(S) % 6
    rng = np.random.default_rng(17)
    scores = (np.round(rng.standard_normal(int(lengths.sum())) * 2) / 2).astype(np.float32)
    _check_topk(eng, scores, _ptr_of(lengths), k)


# ---- recommend end to end against pure numpy -----------------------------------------------------------------------------
def _hash_scores(u, v):
    """An integer hash of the pair modulo 11, as fp32: many ties.  The same expression on int64 tensors and arrays."""
    return ((u * 2654435761 + v * 40503) >> 7) % 11


@pytest.mark.parametrize("cap", [1, 257, 1 << 20])
def test_recommend_is_candidates_scores_topk_in_numpy(hub, cap):
    from s3grl_amd import recommend as R

    A, ids, _, g = hub(4097)
    k, hops = 10, 3
    sources = [ids["s"], ids["hub_big"], ids["iso0"], ids["hub17"], ids["s"], ids["hub128"], ids["iso1"], ids["x"],
               ids["hub65"], 7, ids["hub_big"], ids["hub16"]]
    plain_ptr, plain = ref.candidates(A, sources, hops)
    exclude = np.array([[ids["s"]] * 4 + [ids["hub_big"], 7], plain[:4].tolist() + [int(plain[plain_ptr[1] + 5]), 7]])
    calls = []

    def scorer(pairs):
        assert pairs.dtype == torch.int64 and pairs.is_cuda and pairs.shape[0] == 2 and pairs.shape[1] > 0
        calls.append(pairs.shape[1])
        return _hash_scores(pairs[0], pairs[1]).to(torch.float32)

    top = R.recommend(g, sources, scorer, k=k, hops=hops, exclude=exclude, chunk_pairs=cap)
    ptr, cand = ref.candidates(A, sources, hops, exclude)
    src_of = np.repeat(np.asarray(sources, dtype=np.int64), np.diff(ptr))
    scores = _hash_scores(src_of, cand.astype(np.int64)).astype(np.float32)
    assert 10000 < ptr[-1] <= plain_ptr[-1] - 2 * 4 - 2 * 1 and len(np.unique(scores)) == 11
    nodes, vals, count = ref.segment_topk(scores, ptr, cand, k)
    assert np.array_equal(top.nodes.cpu().numpy(), nodes) and np.array_equal(top.count.cpu().numpy(), count)
    assert np.array_equal(top.scores.cpu().numpy().view(np.int32), vals.view(np.int32))
    assert sum(calls) == ptr[-1] and (len(calls) == 1) == (cap == 1 << 20)
    assert count.tolist()[2] == 0 and count.tolist()[6] == 0 and np.array_equal(nodes[0], nodes[4])
