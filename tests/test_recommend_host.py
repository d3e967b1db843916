"""Link recommendation without a GPU: the numpy restatement against scipy's shortest paths and hand-worked cases, the
candidate kernel's layout, the C ABI's new symbols and limits, every argument error the host can detect, and what the
case builders of tests/recommend_cases.py promise to tests/test_gpu_recommend_shapes.py."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy.sparse.csgraph import shortest_path

import recommend_cases as cases
import recommend_reference as ref
from conftest import load_extract
from s3grl_amd import _native, recommend as R

REPO = Path(__file__).resolve().parent.parent
SYMBOLS = {"s3grl_candidates_layout", "s3grl_candidates_count", "s3grl_candidates_fill", "s3grl_segment_topk"}


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rand300", "usair"])
@pytest.mark.parametrize("hops", [2, 3])
def test_reference_candidates_are_scipy_distances(name, hops):
    z = load_extract(name)
    n = int(z["num_nodes"])
    A = ref.csr_of(n, z["edges"])
    dist = shortest_path(A, method="D", unweighted=True)
    seg_ptr, cand = ref.candidates(A, np.arange(n), hops)
    assert seg_ptr[0] == 0 and seg_ptr[-1] == len(cand) and cand.dtype == np.int32
    for u in range(n):
        want = np.nonzero((dist[u] >= 2) & (dist[u] <= hops))[0]
        assert np.array_equal(cand[seg_ptr[u]:seg_ptr[u + 1]], want), u


def test_reference_candidates_exclude_and_repeats():
    A = ref.csr_of(5, [(0, 1), (1, 2), (2, 3), (3, 4)])                       # a path
    seg_ptr, cand = ref.candidates(A, [0, 4, 0], 3)
    assert seg_ptr.tolist() == [0, 2, 4, 6] and cand.tolist() == [2, 3, 1, 2, 2, 3]
    seg_ptr, cand = ref.candidates(A, [0, 2], 4, exclude=[[3, 4, 0, 1], [0, 2, 4, 0]])   # (3,0) (4,2) (0,4) (1,0)
    assert seg_ptr.tolist() == [0, 1, 2] and cand.tolist() == [2, 0]


def test_reference_topk_is_the_lexsort_rule():
    s = np.array([1.0, np.nan, 2.0, 2.0, -np.inf, np.inf, -0.0, 0.0, 1.0], dtype=np.float32)
    assert ref.segment_order(s).tolist() == [5, 2, 3, 0, 8, 6, 7, 4, 1]
    finite = s[~np.isnan(s)]
    assert np.array_equal(ref.segment_order(finite), np.lexsort((np.arange(len(finite)), -finite)))
    cand = np.arange(10, 19, dtype=np.int32)
    nodes, top, count = ref.segment_topk(s, np.array([0, 0, 3, 9]), cand, 4)
    assert count.tolist() == [0, 3, 4]
    assert nodes.tolist() == [[-1] * 4, [12, 10, 11, -1], [15, 13, 18, 16]]
    assert np.array_equal(top[1], np.array([2.0, 1.0, np.nan, -np.inf], dtype=np.float32), equal_nan=True)
    assert np.all(np.isneginf(top[0]))


# ---- the layout --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,flavour,words", [(1, "lds", 1), (32, "lds", 1), (33, "lds", 2), (524288, "lds", 16384),
                                             (524289, "hbm", 16385)])
def test_layout_switches_flavour_at_the_lds_bound(n, flavour, words):
    lay = R.layout(n, 2)
    assert lay["bitmap"] == flavour and lay["bitmap_words"] == words and lay["lds_nodes"] == 524288
    assert lay["threads"] in (64, 256, 1024) and lay["threads"] == R.layout(n, 8)["threads"]
    if flavour == "lds":
        assert lay["lds_bytes"] == 8 * words <= 160 * 1024 and lay["workspace_bytes"] == 0
        assert lay["resident_workgroups"] == 0
    else:
        assert lay["lds_bytes"] == 0 and lay["workspace_bytes"] == 8 * words and lay["resident_workgroups"] > 0


def test_layout_argument_errors():
    for bad in (0, -1, 1 << 31, 2.0, True):
        with pytest.raises(ValueError, match="num_nodes"):
            R.layout(bad)
    for bad in (1, 0, 9, 2.0):
        with pytest.raises(ValueError, match="hops"):
            R.layout(100, bad)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_[a-z_]+)\s*\(", header))
    assert SYMBOLS <= declared and SYMBOLS <= set(_native.SYMBOLS)
    lib = _native.lib()
    for name in SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.s3grl_abi_version() == 6


def test_limits_through_the_c_abi():
    lib, null = _native.lib(), C.c_void_p(0)
    assert lib.s3grl_segment_topk(null, null, null, null, 0, 0, 1025, null, null, null) == _native.ERR_NOT_IMPLEMENTED
    assert b"1024" in lib.s3grl_last_error()
    with pytest.raises(NotImplementedError, match="1024"):
        _native.check(_native.ERR_NOT_IMPLEMENTED, "s3grl_segment_topk")
    assert lib.s3grl_segment_topk(null, null, null, null, 0, 0, 0, null, null, null) == _native.ERR_INVALID_ARGUMENT
    assert lib.s3grl_segment_topk(null, null, null, null, 0, 0, 10, null, null, null) == _native.ERR_INVALID_ARGUMENT
    total = C.c_int64()
    for hops in (9, 1):
        assert lib.s3grl_candidates_count(null, null, null, 0, hops, null, 0, null,
                                          C.byref(total)) == _native.ERR_INVALID_ARGUMENT
        assert b"hops" in lib.s3grl_last_error()
        assert lib.s3grl_candidates_fill(null, null, null, 0, hops, null, 0, null, null) == _native.ERR_INVALID_ARGUMENT
    assert lib.s3grl_candidates_count(null, null, null, 0, 2, null, 0, null,
                                      C.byref(total)) == _native.ERR_INVALID_ARGUMENT      # no context, no graph
    out = (C.c_int64 * 8)()
    assert lib.s3grl_candidates_layout(0, 2, out) == _native.ERR_INVALID_ARGUMENT
    assert lib.s3grl_candidates_layout(10, 9, out) == _native.ERR_INVALID_ARGUMENT
    assert lib.s3grl_candidates_layout(10, 2, None) == _native.ERR_INVALID_ARGUMENT


# ---- argument errors of the Python layer, all before any GPU work -----------------------------------------------------
GRAPH = SimpleNamespace(num_nodes=10, directed=False)      # never reached: every call below fails in its checks


def _scorer(pairs):
    raise AssertionError("the scorer must not run")


@pytest.mark.parametrize("call", [lambda **kw: R.candidates(GRAPH, **kw),
                                  lambda **kw: R.recommend(GRAPH, scorer=_scorer, **kw)])
def test_candidate_argument_errors(call):
    for hops in (1, 0, -2, 2.0, 9):
        with pytest.raises(ValueError, match="hops"):
            call(sources=[0, 1], hops=hops)
    for sources in ([0.0, 1.0], torch.tensor([0.5]), np.array([True, False])):
        with pytest.raises(ValueError, match="sources"):
            call(sources=sources)
    for sources in ([0, 10], [-1], torch.tensor([3, 11]), np.array([[0, 1]])):
        with pytest.raises(ValueError, match="sources"):
            call(sources=sources)
    for exclude in (np.zeros((3, 2), dtype=np.int64), np.zeros(4, dtype=np.int64), torch.zeros((2, 3, 1), dtype=torch.int64),
                    np.zeros((2, 2)), np.array([[0, 1], [2, 10]])):
        with pytest.raises(ValueError, match="exclude"):
            call(sources=[0, 1], exclude=exclude)


def test_recommend_argument_errors():
    for k in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="k must"):
            R.recommend(GRAPH, [0], _scorer, k=k)
    for cap in (0, -5, 1.0):
        with pytest.raises(ValueError, match="chunk_pairs"):
            R.recommend(GRAPH, [0], _scorer, chunk_pairs=cap)
    with pytest.raises(ValueError, match="kind"):
        R.HeuristicScorer(None, "PPR")


def test_segment_topk_argument_errors():
    seg_ptr, cand = torch.tensor([0, 2, 5]), torch.arange(5, dtype=torch.int32)
    good = torch.zeros(5)
    for k in (0, -3, 2.0):
        with pytest.raises(ValueError, match="k must"):
            R.segment_topk(good, seg_ptr, cand, k)
    for scores in (torch.zeros(4), torch.zeros(6), torch.zeros((5, 1)), torch.zeros(5, dtype=torch.float64),
                   torch.zeros(5, dtype=torch.int32), np.zeros(5, dtype=np.float32)):
        with pytest.raises(ValueError, match="scores"):
            R.segment_topk(scores, seg_ptr, cand, 3)
    with pytest.raises(ValueError, match="seg_ptr"):
        R.segment_topk(good, seg_ptr.to(torch.int32), cand, 3)
    with pytest.raises(ValueError, match="cand"):
        R.segment_topk(good, seg_ptr, cand.long(), 3)


# ---- host helpers ------------------------------------------------------------------------------------------------------
def test_chunks_are_consecutive_and_within_the_cap():
    ptr = np.array([0, 3, 3, 10, 11, 11, 40, 41], dtype=np.int64)      # lengths 3 0 7 1 0 29 1
    assert R._chunks(ptr, 1 << 20) == [(0, 7)]
    assert R._chunks(ptr, 10) == [(0, 3), (3, 5), (5, 6), (6, 7)]      # 29 > 10: a chunk of its own
    assert R._chunks(ptr, 1) == [(0, 1), (1, 2), (2, 3), (3, 5), (5, 6), (6, 7)]
    assert R._chunks(np.array([0], dtype=np.int64), 5) == []
    for cap in (1, 2, 7, 8, 30, 41):
        ch = R._chunks(ptr, cap)
        assert ch[0][0] == 0 and ch[-1][1] == 7 and all(p[1] == q[0] for p, q in zip(ch, ch[1:]))
        assert all(b - a == 1 or ptr[b] - ptr[a] <= cap for a, b in ch)


def test_recall_at_k_by_hand():
    top = R.TopK(torch.tensor([[5, 6, -1], [7, 8, 9], [1, 2, 3]], dtype=torch.int32), torch.zeros((3, 3)),
                 torch.tensor([2, 3, 3], dtype=torch.int32))
    sources = [0, 4, 0]                                                # node 0 twice: its first row counts
    targets = np.array([[0, 0, 4, 4, 2, 0], [5, 1, 9, 0, 7, 6]])       # (2, 7): 2 is no source
    assert R.recall_at_k(top, sources, targets) == pytest.approx(3 / 5)
    assert np.isnan(R.recall_at_k(top, sources, np.array([[2], [7]])))
    with pytest.raises(ValueError, match="targets"):
        R.recall_at_k(top, sources, np.zeros((3, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="sources"):
        R.recall_at_k(top, [0, 4], targets)


# ---- the case builders of tests/recommend_cases.py: what the GPU tests rely on -------------------------------------------
@pytest.fixture(scope="module", params=cases.HUB_SIZES)
def hub(request):
    return cases.hub_graph(request.param)


def test_hub_graph_is_a_sorted_symmetric_csr_with_the_promised_rows(hub):
    A, ids, rows = hub
    n = A.shape[0]
    assert (A != A.T).nnz == 0 and A.has_sorted_indices and A.diagonal().sum() == 0
    assert all(np.all(np.diff(A.indices[A.indptr[v]:A.indptr[v + 1]]) > 0) for v in ids.values())
    assert {name: rows[name] for name in cases.HUB_ROWS} == cases.HUB_ROWS
    assert sorted(cases.HUB_ROWS.values())[:8] == [15, 16, 17, 63, 64, 65, 128, 129] and cases.HUB_ROWS["hub_big"] > 1024
    assert sorted(cases.hub_names(ids)) == sorted(cases.HUB_ROWS)
    assert rows["s"] == 1 and rows["x"] == len(cases.HUB_ROWS) + 1
    assert [rows[name] for name in cases.isolated_names(ids)] == [0, 0, 0]
    assert ids["hub_big"] == 0 and ids["hub128"] == n - 1
    # two long rows in one frontier word; two in different lanes of one 64-word chunk
    assert ids["hub17"] >> 5 == ids["hub65"] >> 5 and min(rows["hub17"], rows["hub65"]) > 16
    assert ids["hub64"] >> 11 == ids["hub129"] >> 11 and ids["hub64"] >> 5 != ids["hub129"] >> 5
    assert min(rows["hub64"], rows["hub129"]) > 16
    # the hubs' neighbours reach the first and the last bitmap word and every 64-word chunk between
    nb = np.concatenate([A.indices[A.indptr[ids[h]]:A.indptr[ids[h] + 1]] for h in cases.hub_names(ids)])
    assert (nb >> 5).max() == (n - 1) >> 5 and (nb >> 5).min() == 0
    assert len(np.unique(nb >> 11)) == ((n - 1) >> 11) + 1


def test_hub_graph_frontiers_of_s(hub):
    A, ids, _ = hub
    dist = shortest_path(A, method="D", unweighted=True, indices=[ids["s"]])[0]
    hubs = sorted(ids[h] for h in cases.hub_names(ids))
    assert np.nonzero(dist == 1)[0].tolist() == [ids["x"]]
    assert np.nonzero(dist == 2)[0].tolist() == hubs                    # level 2's frontier: every hub and nothing else
    assert all(np.isinf(dist[ids[name]]) for name in cases.isolated_names(ids))


@pytest.mark.parametrize("n,flavour,threads,words", [(4096, "lds", 64, 128), (4097, "lds", 256, 129),
                                                     (131073, "lds", 1024, 4097), (524289, "hbm", 1024, 16385)])
def test_hub_graph_sizes_reach_every_instantiation(n, flavour, threads, words):
    lay = R.layout(n)
    assert n in cases.HUB_SIZES
    assert (lay["bitmap"], lay["threads"], lay["bitmap_words"]) == (flavour, threads, words)
    assert (lay["resident_workgroups"] > 0) == (flavour == "hbm")
    assert words > 64 and (words % 64 == 1 or n == 4096)                # a last chunk of one live lane, or two full ones


def test_star_and_paths():
    A = cases.star(7)
    assert A.shape == (7, 7) and np.diff(A.indptr).tolist() == [6] + [1] * 6
    assert cases.path(4).toarray().tolist() == [[0, 1, 0, 0], [1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 1, 0]]
    B = cases.two_paths(3, 4)
    assert B.shape == (7, 7) and B.nnz == 2 * (2 + 3) and B[:3, 3:].nnz == 0 and B[2, 3] == 0
    assert np.diff(B.indptr).tolist() == [1, 2, 1, 1, 2, 2, 1]


def test_candidates_tiled_is_the_reference():
    z = load_extract("rand300")
    A = ref.csr_of(300, z["edges"])
    sources, ex = [7, 3, 7, 299, 0, 3, 3], np.array([[7, 3], [20, 9]])
    for exclude in (None, ex):
        want_ptr, want = ref.candidates(A, sources, 3, exclude)
        got_ptr, got = cases.candidates_tiled(A, sources, 3, exclude)
        assert got_ptr.dtype == np.int64 and got.dtype == np.int32
        assert np.array_equal(got_ptr, want_ptr) and np.array_equal(got, want)
    ptr, cand = cases.candidates_tiled(A, [], 2)
    assert ptr.tolist() == [0] and len(cand) == 0


def test_stride_sources_alternate_kinds_within_every_workgroup():
    info = cases.hub_graph(524289)
    A, ids, _ = info
    resident, rounds, hops = R.layout(524289)["resident_workgroups"], 2, 3
    sources, kinds = cases.stride_sources(info, resident, rounds, hops)
    assert len(sources) == rounds * resident + 5 == len(kinds)
    for i in range(resident):
        mine = kinds[i::resident]
        assert len(mine) >= rounds and np.all(mine[1:] != mine[:-1]), i
    assert {tuple(kinds[i::resident]) for i in range(5)} >= {(0, 1, 2), (1, 2, 0), (2, 0, 1)}   # three in turn
    # the kinds are what they say: ball sizes from the restatement
    ptr, _ = cases.candidates_tiled(A, sources, hops)
    size = np.diff(ptr)
    assert np.all(size[kinds == cases.EMPTY] == 0) and np.all(size[kinds == cases.LARGE] > 1000)
    assert np.all((size[kinds == cases.TINY] > 0) & (size[kinds == cases.TINY] < 64))
    deg = np.diff(A.indptr)
    assert np.all(deg[sources[kinds == cases.TINY]] >= 2) and len(np.unique(sources[kinds == cases.TINY])) > 32


def test_order_key_restated():
    s = np.array([np.inf, 1.0, 1e-45, 0.0, -0.0, -1e-45, -1.0, -np.inf, np.nan, -np.nan], dtype=np.float32)
    key = cases.order_key(s)
    assert key.dtype == np.uint32 and np.all(np.diff(key[:4].astype(np.int64)) < 0) and key[3] == key[4]
    assert np.all(np.diff(key[4:9].astype(np.int64)) < 0) and key[8] == key[9] == 0 and key[7] > 0
    rng = np.random.default_rng(2)
    f = cases.any_finite(4000, rng)
    a, b = f[:2000], f[2000:]
    assert np.array_equal(cases.order_key(a) > cases.order_key(b), a > b)      # order-preserving on the non-NaNs


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("digit", [0, 1, 2, 3])
def test_digit_scores_share_the_bits_above_the_digit(digit, negative):
    s = cases.digit_scores(5000, digit, np.random.default_rng(digit), negative)
    key = cases.order_key(s).astype(np.uint64)
    assert not np.isnan(s).any() and np.all(np.signbit(s) == negative)
    assert len(np.unique(key >> (8 * (digit + 1)))) == 1                      # agree above the digit
    assert len(np.unique((key >> (8 * digit)) & 255)) > 64                    # vary inside it
    assert 2 < len(np.unique(key)) < 5000 // 2                                # ties exist


@pytest.mark.parametrize("kind", [("digit", d, neg) for d in (0, 1, 2, 3) for neg in (False, True)])
def test_select_case_has_a_tie_across_every_cut(kind):
    s = cases.select_case(kind, seed=4)
    assert len(s) == sum(cases.SELECT_LENGTHS) and {2049, 4097, 10000} <= set(cases.SELECT_LENGTHS)
    a = 0
    for n in cases.SELECT_LENGTHS:
        key = np.sort(cases.order_key(s[a:a + n]))[::-1]
        assert len(np.unique(key.astype(np.uint64) >> (8 * (kind[1] + 1)))) == 1
        for k in cases.SELECT_KS:
            assert k >= n or key[k - 1] == key[k], (n, k)
        a += n


def test_any_finite_covers_the_classes():
    s = cases.any_finite(3000, np.random.default_rng(0))
    u = s.view(np.uint32)
    assert not np.isnan(s).any()
    for pattern in (0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x80000001):
        assert (u == pattern).sum() >= 2
    denormal = ((u & 0x7f800000) == 0) & ((u & 0x007fffff) != 0)
    assert denormal.sum() >= 8 and np.signbit(s).sum() > 1000 and (~np.signbit(s)).sum() > 1000


@pytest.mark.parametrize("keep", [0, 1, 5, 2999, 3000])
def test_nan_heavy_keeps_exactly(keep):
    s = cases.nan_heavy(3000, keep, np.random.default_rng(keep))
    assert int((~np.isnan(s)).sum()) == keep
    nan_bits = s.view(np.uint32)[np.isnan(s)]
    if len(nan_bits) > 100:
        assert len(np.unique(nan_bits)) > 50 and len(np.unique(nan_bits >> 31)) == 2   # payloads and signs vary


@pytest.mark.parametrize("k", [64, 1000])
@pytest.mark.parametrize("where", ["head", "tail", "spread"])
def test_ties_at_puts_the_ties_where_it_says(where, k):
    n, chunks = 6000, -(-6000 // 256)
    for r in (1, 7, k):
        s, pos = cases.ties_at(n, k, r, where)
        assert np.array_equal(np.nonzero(s == 1.0)[0], pos) and len(pos) > r      # more ties than the cut takes
        assert int((s == 2.0).sum()) == k - r and set(np.unique(s)) <= {0.0, 1.0, 2.0}
        first = pos[:r]
        if where == "head":
            assert first.tolist() == list(range(r)) and (r > 200 or pos[-1] < 256)
        elif where == "tail":
            assert pos[-1] == n - 1 and first[0] == n - len(pos) and (r > 200 or first[0] >= n - 256)
        elif len(pos) <= chunks:
            assert np.array_equal(pos >> 8, np.arange(len(pos)))                 # one per 256-position chunk
        else:
            per = np.bincount(pos >> 8, minlength=chunks)
            assert per.max() - per.min() <= 1 and per.min() > 0                  # dealt round every chunk
        # the restatement takes the 2.0s and then exactly the first r ties
        order = ref.segment_order(s)[:k]
        assert np.array_equal(np.sort(order[k - r:]), first) and np.all(s[order[:k - r]] == 2.0)


def test_reference_topk_agrees_with_a_plain_sort():
    s = cases.any_finite(300, np.random.default_rng(7))
    s[[3, 50, 299]] = np.nan
    s[[10, 11, 200]] = s[10]                                                   # a three-way tie

    def rule(j):                                                                # the documented rule, spelled out
        v = float(s[j])
        return (1, 0.0, j) if v != v else (0, -(v + 0.0), j)

    want = sorted(range(300), key=rule)
    assert ref.segment_order(s).tolist() == want
    nodes, top, count = ref.segment_topk(s, np.array([0, 300]), np.arange(300, dtype=np.int32), 300)
    assert nodes[0].tolist() == want and count.tolist() == [300]
    assert np.array_equal(top[0].view(np.uint32), s[want].view(np.uint32))


def test_empty_source_list_passes_the_host_checks():
    for empty in ([], (), np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int32)):
        assert R._check_sources(empty, 10).numel() == 0
    for bad in (np.zeros(0), torch.zeros(0)):                                   # an explicit float dtype stays an error
        with pytest.raises(ValueError, match="sources"):
            R._check_sources(bad, 10)
