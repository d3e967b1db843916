"""Link recommendation on the MI355X (s3grl_amd.recommend): the candidate kernel and the segment top-K against their
numpy restatement (tests/recommend_reference.py), exactly; their limits; and USAir end to end.  Every shape is the
smallest at which its piece can go wrong: word edges of the bitmaps, segments around a wavefront, a workgroup and the
in-LDS sort (2 048 entries), the switch to bitmaps in HBM (524 289 nodes)."""
import numpy as np
import pytest
import torch

import recommend_reference as ref
from conftest import load_extract

pytestmark = pytest.mark.gpu

LDS_SORT = 2048          # kTopSort of csrc/s3grl_recommend.hip: longer segments go through the radix select


@pytest.fixture(scope="module")
def eng():
    from s3grl_amd.engine import default_engine

    return default_engine("cuda:0")


def _check_candidates(eng, A, sources, hops, exclude=None):
    from s3grl_amd import recommend as R

    g = eng.graph(A)
    try:
        seg_ptr, cand = R.candidates(g, sources, hops, exclude)
    finally:
        g.close()
    assert seg_ptr.dtype == torch.int64 and cand.dtype == torch.int32 and seg_ptr.is_cuda and cand.is_cuda
    want_ptr, want = ref.candidates(A, sources, hops, exclude)
    assert np.array_equal(seg_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(cand.cpu().numpy(), want)
    return want_ptr, want


def _ring(n, chord_every, chord):
    i = np.arange(n, dtype=np.int64)
    c = i[::chord_every]
    return ref.csr_of(n, np.concatenate([np.stack([i, (i + 1) % n], 1), np.stack([c, (c + chord) % n], 1)]))


# ---- candidates ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hops", [2, 3, 4])
def test_path_of_five(eng, hops):
    A = ref.csr_of(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    ptr, cand = _check_candidates(eng, A, np.arange(5), hops)
    assert cand[ptr[0]:ptr[1]].tolist() == list(range(2, hops + 1))             # the end node: level bookkeeping


def test_star_of_300_leaves(eng):
    A = ref.csr_of(301, [(0, v) for v in range(1, 301)])
    ptr, _ = _check_candidates(eng, A, np.arange(301), 2)
    assert np.diff(ptr).tolist() == [0] + [299] * 300                            # longer than a wavefront and than 256


def test_empty_segments_at_the_start_middle_and_end(eng):
    tri = [(0, 1), (1, 2), (0, 2)]                                               # node 3 is isolated
    ptr, _ = _check_candidates(eng, ref.csr_of(4, tri), np.arange(4), 3)
    assert ptr.tolist() == [0] * 5
    A = ref.csr_of(7, tri + [(4, 5), (5, 6)])
    ptr, cand = _check_candidates(eng, A, [3, 4, 0, 6, 3], 2)
    assert np.diff(ptr).tolist() == [0, 1, 0, 1, 0] and cand.tolist() == [6, 4]


@pytest.mark.parametrize("name", ["rand300", "usair"])
@pytest.mark.parametrize("hops", [2, 3])
def test_every_node_of_a_real_graph(eng, name, hops):
    z = load_extract(name)
    n = int(z["num_nodes"])
    _check_candidates(eng, ref.csr_of(n, z["edges"]), np.arange(n), hops)


def test_repeated_and_unordered_sources(eng):
    z = load_extract("rand300")
    ptr, cand = _check_candidates(eng, ref.csr_of(300, z["edges"]), [7, 3, 7, 299, 0, 3], 2)
    assert np.array_equal(cand[ptr[0]:ptr[1]], cand[ptr[2]:ptr[3]]) and ptr[1] > 0


def test_exclusion_rule(eng):
    z = load_extract("rand300")
    A = ref.csr_of(300, z["edges"])
    sources = [5, 17, 40]
    ptr, cand = ref.candidates(A, sources, 2)
    _, far = ref.candidates(A, [5], 4)
    beyond = int(np.setdiff1d(far, cand[ptr[0]:ptr[1]])[0])                      # a node 3 or 4 hops from 5
    nbr = int(A.indices[A.indptr[17]])                                           # an edge
    mid = int(cand[(ptr[1] + ptr[2]) // 2])
    pairs = [(5, int(cand[ptr[0]])), (int(cand[ptr[1] - 1]), 5),                 # the first and last candidate of 5
             (17, mid), (mid, 17), (17, mid),                                    # both orientations, and a duplicate
             (17, nbr), (5, beyond)]
    got_ptr, got = _check_candidates(eng, A, sources, 2, np.array(pairs, dtype=np.int64).T)
    assert np.diff(got_ptr).tolist() == [ptr[1] - ptr[0] - 2, ptr[2] - ptr[1] - 1, ptr[3] - ptr[2]]
    assert mid not in got[got_ptr[1]:got_ptr[2]]


@pytest.mark.parametrize("n", [33, 65])
@pytest.mark.parametrize("hops", [2, 3])
def test_word_edges_of_the_bitmap(eng, n, hops):
    ptr, cand = _check_candidates(eng, _ring(n, 8, 5), np.arange(n), hops)
    assert n - 1 in cand and n - 2 in cand[ptr[0]:ptr[1]]                        # the last word's only bit(s)


def test_bitmaps_in_hbm_beyond_the_lds_bound(eng):
    from s3grl_amd import recommend as R

    n = 524289
    assert R.layout(n)["bitmap"] == "hbm" and R.layout(n - 1)["bitmap"] == "lds"
    A = _ring(n, 64, 12345)
    sources = [0, n - 1, 64, 12345, 262144, 524224, 31, n - 1]
    ptr, cand = _check_candidates(eng, A, sources, 3, np.array([[0, 2], [2, n - 1]]))
    assert np.array_equal(cand[ptr[1]:ptr[2]], cand[ptr[7]:ptr[8]]) and 1 in cand[ptr[1]:ptr[2]]
    assert 2 not in cand[ptr[0]:ptr[1]] and 2 not in cand[ptr[1]:ptr[2]]


# 64 threads up to 128 bitmap words, 256 up to 4 096, 1 024 beyond; 524 288 nodes: the largest bitmaps LDS holds
@pytest.mark.parametrize("n", [4096, 4097, 131072, 131073, 524288])
def test_every_workgroup_size_of_the_lds_flavour(eng, n):
    from s3grl_amd import recommend as R

    assert R.layout(n)["threads"] == {4096: 64, 4097: 256, 131072: 256, 131073: 1024, 524288: 1024}[n]
    _check_candidates(eng, _ring(n, 64, 1234), [0, n - 1, 64, n // 2, 1234], 3, np.array([[n - 1], [1]]))


def test_a_second_run_is_bit_identical(eng):
    from s3grl_amd import recommend as R

    z = load_extract("rand300")
    g = eng.graph(ref.csr_of(300, z["edges"]))
    ex = torch.tensor([[1, 2, 3], [9, 8, 7]])
    a = R.candidates(g, np.arange(300), 3, ex)
    b = R.candidates(g, np.arange(300), 3, ex)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    g.close()


# ---- segment top-K ------------------------------------------------------------------------------------------------------
def _lengths(k):
    base = [0, 1, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, LDS_SORT - 1, LDS_SORT, LDS_SORT + 1, 5000, 0]
    return [0] + [x for x in base if x >= 0]          # an empty segment at the start, in the middle and at the end


def _scores(kind, lengths, k, rng):
    P = int(np.sum(lengths))
    if kind == "normal":
        return rng.standard_normal(P).astype(np.float32)
    if kind == "all_equal":
        return np.full(P, 0.25, dtype=np.float32)
    if kind == "two_valued":                           # the cut falls inside a tie group in every segment longer than k
        return (rng.random(P) < 0.4).astype(np.float32)
    if kind == "quantised":                            # ties inside every digit of the radix select
        return (np.round(rng.standard_normal(P) * 4) / 4).astype(np.float32)
    assert kind == "special"
    s = rng.standard_normal(P).astype(np.float32)
    pick = rng.random(P)
    s[pick < 0.10] = np.inf
    s[(pick >= 0.10) & (pick < 0.20)] = -np.inf
    s[(pick >= 0.20) & (pick < 0.35)] = -0.0
    s[(pick >= 0.35) & (pick < 0.50)] = 0.0
    return s


def _check_topk(eng, scores, lengths, k, offset=0):
    from s3grl_amd import recommend as R

    seg_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    P = int(seg_ptr[-1])
    cand = np.random.default_rng(5).integers(0, 1 << 30, P).astype(np.int32)
    buf = torch.zeros(P + offset, dtype=torch.float32, device=eng.device)
    buf[offset:] = torch.as_tensor(scores)
    s_dev = buf[offset:]
    assert offset == 0 or s_dev.data_ptr() % 16 != 0
    top = R.segment_topk(s_dev, torch.as_tensor(seg_ptr).to(eng.device), torch.as_tensor(cand).to(eng.device), k,
                         engine=eng)
    read_back = s_dev.cpu().numpy()
    nodes, vals, count = ref.segment_topk(read_back, seg_ptr, cand, k)
    assert top.nodes.dtype == torch.int32 and top.scores.dtype == torch.float32 and top.count.dtype == torch.int32
    assert np.array_equal(top.count.cpu().numpy(), count)
    assert np.array_equal(top.count.cpu().numpy(), np.minimum(k, lengths))
    assert np.array_equal(top.nodes.cpu().numpy(), nodes)
    assert np.array_equal(top.scores.cpu().numpy().view(np.int32), vals.view(np.int32))      # bit for bit
    return top


@pytest.mark.parametrize("k", [1, 10, 64, 1024])
@pytest.mark.parametrize("kind", ["normal", "all_equal", "two_valued", "quantised", "special"])
def test_topk_is_the_lexsort(eng, kind, k):
    lengths = _lengths(k)
    _check_topk(eng, _scores(kind, lengths, k, np.random.default_rng(k)), lengths, k)


@pytest.mark.parametrize("k", [1, 10, 64, 1024])
def test_topk_one_nan_in_a_segment_of_k_plus_one(eng, k):
    rng = np.random.default_rng(3)
    lengths = [k + 1, k + 1, LDS_SORT + k + 1]
    s = rng.standard_normal(int(np.sum(lengths))).astype(np.float32)
    s[k // 2] = np.nan                                   # ranks last: it alone is cut
    s[k + 1] = -np.inf
    s[k + 2] = np.nan                                    # a NaN next to -inf: -inf is kept, the NaN is cut
    s[2 * (k + 1) + 7] = np.nan
    top = _check_topk(eng, s, lengths, k)
    assert not bool(torch.isnan(top.scores).any())


def test_topk_nans_fill_up_short_segments(eng):
    s = np.array([np.nan, 1.0, np.nan, -np.inf, np.nan, np.nan], dtype=np.float32)
    top = _check_topk(eng, s, [4, 2], 3)
    assert top.nodes.shape == (2, 3) and int(top.nodes[1, 2]) == -1 and bool(torch.isneginf(top.scores[1, 2]))


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_topk_scores_that_start_off_a_16_byte_boundary(eng, offset):
    lengths = [257, 3, LDS_SORT + 1]
    _check_topk(eng, _scores("normal", lengths, 10, np.random.default_rng(offset)), lengths, 10, offset=offset)


def test_topk_one_long_segment(eng):
    lengths = [70001]
    for kind in ("quantised", "all_equal"):
        _check_topk(eng, _scores(kind, lengths, 1024, np.random.default_rng(9)), lengths, 1024)


def test_topk_many_long_segments_at_once(eng):
    """Every CU busy with several radix selects: the passes of a select hand their digit over through LDS, and a
    wavefront that runs late must still read its own pass's."""
    lengths = [LDS_SORT + 1 + 7 * (i % 50) for i in range(1200)]
    for kind, k in (("quantised", 64), ("two_valued", 1024)):
        _check_topk(eng, _scores(kind, lengths, k, np.random.default_rng(11)), lengths, k)


def test_topk_a_second_run_is_bit_identical(eng):
    from s3grl_amd import recommend as R

    lengths = _lengths(64)
    s = torch.as_tensor(_scores("quantised", lengths, 64, np.random.default_rng(1))).to(eng.device)
    seg_ptr = torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(eng.device)
    cand = torch.arange(s.numel(), dtype=torch.int32, device=eng.device)
    a, b = R.segment_topk(s, seg_ptr, cand, 64, engine=eng), R.segment_topk(s, seg_ptr, cand, 64, engine=eng)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- limits, and the checks behind the ABI -------------------------------------------------------------------------
def test_limits(eng):
    from conftest import csr_from_arcs
    from s3grl_amd import recommend as R

    s, seg_ptr, cand = (torch.zeros(4, device=eng.device), torch.tensor([0, 4], device=eng.device),
                        torch.arange(4, dtype=torch.int32, device=eng.device))
    with pytest.raises(NotImplementedError, match="1024"):
        R.segment_topk(s, seg_ptr, cand, 1025, engine=eng)
    assert R.segment_topk(s, seg_ptr, cand, 1024, engine=eng).count.tolist() == [4]
    g = eng.graph(csr_from_arcs(4, [(0, 1), (1, 2), (2, 3)]), directed=True)
    with pytest.raises(NotImplementedError, match="directed"):
        R.candidates(g, [0], 2)
    with pytest.raises(NotImplementedError, match="directed"):             # and behind the ABI
        R._count(g, torch.zeros(1, dtype=torch.int32, device=eng.device), 2, None)
    g.close()
    g = eng.graph(ref.csr_of(3, [(0, 1), (1, 2)]))
    with pytest.raises(NotImplementedError, match="1024"):
        R.recommend(g, [0], lambda pairs: None, k=1025)
    g.close()


def test_arguments_are_checked_behind_the_abi(eng):
    from s3grl_amd import recommend as R

    g = eng.graph(ref.csr_of(5, [(0, 1), (1, 2), (2, 3), (3, 4)]))
    dev = eng.device
    with pytest.raises(ValueError, match="source"):
        R._count(g, torch.tensor([0, 5], dtype=torch.int32, device=dev), 2, None)
    with pytest.raises(ValueError, match="source"):
        R._count(g, torch.tensor([-1], dtype=torch.int32, device=dev), 2, None)
    src = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    seg_ptr, total = R._count(g, src, 2, None)
    assert seg_ptr.tolist() == [0, 1, 3] and total == 3
    with pytest.raises(ValueError, match="seg_ptr"):                       # not what the count wrote: nothing is written
        R._fill(g, src, 2, None, torch.tensor([0, 2, 3], device=dev), 3)
    s, cand = torch.zeros(6, device=dev), torch.arange(6, dtype=torch.int32, device=dev)
    for bad in ([0, 4, 3], [0, 3, 7], [-1, 3, 6]):
        with pytest.raises(ValueError, match="seg_ptr"):
            R.segment_topk(s, torch.tensor(bad, device=dev), cand, 2, engine=eng)
    g.close()


# ---- USAir end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def usair(eng):
    from s3grl_amd import workloads

    w = workloads.make("usair_pos_k2")
    G, f = eng.graph(w.A), eng.features(w.X)
    yield w, G, f
    G.close()
    f.close()


def test_usair_recommend_with_a_trained_signnet(eng, usair):
    from s3grl_amd import recommend as R
    from s3grl_amd.signnet import SIGNNetTrainer

    w, G, f = usair
    n = w.A.shape[0]
    pos, neg = w.split.links["train"]
    y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
    kw = dict(mode="pos", num_hops=1, sign_k=2)
    res = eng.precompute(G, f, eng.links(np.concatenate([pos, neg], axis=1)), **kw)
    net = SIGNNetTrainer(int(np.prod(res.rows.shape[1:])), hidden=32, lr=2e-3, seed=1, device="cuda:0")
    for _ in range(2):
        net.fit_epoch(res.rows, res.row_ptr, y, 32)
    sources = np.arange(n)
    top = R.recommend(G, sources, R.SignScorer(eng, G, f, net, **kw), k=10, hops=2)
    # the reference path: the same kernels on the same list in one call, then the restatement's top-K
    seg_ptr, cand = R.candidates(G, sources, 2)
    assert int(seg_ptr[-1]) <= 1 << 20                                        # recommend ran as one chunk
    src_of = torch.repeat_interleave(torch.arange(n, device=eng.device), seg_ptr.diff())
    whole = eng.precompute(G, f, torch.stack([src_of, cand.long()], dim=1).contiguous(), **kw)
    scores = net.score(whole.rows, whole.row_ptr).cpu().numpy()
    nodes, vals, count = ref.segment_topk(scores, seg_ptr.cpu().numpy(), cand.cpu().numpy(), 10)
    assert np.array_equal(top.nodes.cpu().numpy(), nodes) and np.array_equal(top.count.cpu().numpy(), count)
    assert np.array_equal(top.scores.cpu().numpy().view(np.int32), vals.view(np.int32))
    assert np.isfinite(scores).all() and len(np.unique(scores)) > 100                    # a trained model, not a constant
    held = w.split.links["test"][0]
    recall = R.recall_at_k(top, sources, np.concatenate([held, held[::-1]], axis=1))
    print("USAir recall@10 of the held-out test links after 2 epochs:", recall)
    assert 0.0 <= recall <= 1.0
    net.close()


def test_usair_chunking_does_not_change_the_result(eng, usair):
    from s3grl_amd import recommend as R
    from s3grl_amd.heuristics import Heuristics

    w, G, _ = usair
    n = w.A.shape[0]
    h = Heuristics(w.A, device="cuda:0")
    sources = np.arange(n)
    seg_ptr, cand = R.candidates(G, sources, 2)
    src_of = torch.repeat_interleave(torch.arange(n, device=eng.device), seg_ptr.diff())
    full = h.cn(torch.stack([src_of, cand.long()])).cpu().numpy()
    nodes, vals, count = ref.segment_topk(full, seg_ptr.cpu().numpy(), cand.cpu().numpy(), 10)
    assert len(np.unique(full)) > 3 and int(seg_ptr[-1]) > 1000               # ties inside segments, several chunks
    for cap in (1, 1000, 1 << 20):
        top = R.recommend(G, sources, R.HeuristicScorer(h, "CN"), k=10, hops=2, chunk_pairs=cap)
        assert np.array_equal(top.nodes.cpu().numpy(), nodes), cap
        assert np.array_equal(top.scores.cpu().numpy(), vals), cap
        assert np.array_equal(top.count.cpu().numpy(), count), cap
    h.close()


def test_scores_of_the_wrong_length_or_dtype(eng, usair):
    from s3grl_amd import recommend as R

    _, G, _ = usair
    for scorer in (lambda p: torch.zeros(p.shape[1] + 1, device=eng.device),
                   lambda p: torch.zeros(p.shape[1], dtype=torch.float64, device=eng.device),
                   lambda p: np.zeros(p.shape[1], dtype=np.float32)):
        with pytest.raises(ValueError, match="scores"):
            R.recommend(G, [0, 1], scorer, k=3)


def test_recall_at_k_on_a_hand_made_topk(eng):
    from s3grl_amd import recommend as R

    top = R.TopK(torch.tensor([[5, 6, -1], [7, 8, 9]], dtype=torch.int32, device=eng.device),
                 torch.zeros((2, 3), device=eng.device), torch.tensor([2, 3], dtype=torch.int32, device=eng.device))
    targets = torch.tensor([[0, 0, 4, 4, 2], [5, 1, 9, 0, 7]], device=eng.device)
    assert R.recall_at_k(top, torch.tensor([0, 4]), targets) == pytest.approx(2 / 4)
