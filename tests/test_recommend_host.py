"""Link recommendation without a GPU: the numpy restatement against scipy's shortest paths and hand-worked cases, the
candidate kernel's layout, the C ABI's new symbols and limits, and every argument error the host can detect."""
import ctypes as C
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from scipy.sparse.csgraph import shortest_path

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
