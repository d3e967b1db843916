"""The RA / Jaccard / PA / Katz kernels (csrc/s3grl_heuristics.hip: pairs_kernel<kind>, katz_spmm_kernel,
katz_finish_kernel) on the graphs of tests/heuristics_cases.py against the fp64 restatement
(tests/heuristics_more_reference.py; tests/test_heuristics_more_host.py checks it against the definitions and shows
that its named faults leave the bounds used here).

Bounds.  Local indices: bit-equal where every term is an integer, otherwise 1 fp32 ulp of the restatement, plus
1e-13·Σ|term| where terms cancel (DESIGN.md §11's bound).  Katz, per score: 1 fp32 ulp of the restatement +
2·max_len·(m + 3)·2⁻⁵³·KATZ_{|A|,|β|}(s, d) with m the largest stored-entry count of a column (`M.katz_bound`), and
exactly 0 where the restatement is 0.  Every comparison prints how many fp32 results are not bit-equal; that count is
a report, not a threshold.

Calls through the C ABI fill `out` with NaN first: an entry the kernels fail to write cannot pass by holding a right
answer from an earlier call's memory."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import heuristics_cases as K
import heuristics_more_reference as M
import heuristics_reference as R
from test_gpu_heuristics import _split
from test_gpu_heuristics_shapes import _bits, _heur, _layout_pool, _links_to, _np, _same_bits, _sink_case

pytestmark = pytest.mark.gpu

VALUE_SETS = ("A_int", "A_float", "A_signed")
MAX_LENS = (1, 2, 3, 7)                                   # both parities of the buffer the finish reads
BETAS = (0.005, 0.5, -0.5, 1.0)


def _assert_within(what, got, ref, bound):
    """fp32 `got` within `bound` of the fp32 restatement, no NaN, exactly 0 where the restatement is 0"""
    assert got.dtype == np.float32 and got.shape == ref.shape, what
    differ = int(np.count_nonzero(got != ref))
    print(f"[heuristics more] {what}: {differ} of {got.size} fp32 scores not bit-equal to the restatement")
    assert not np.isnan(got).any() and not np.isnan(ref).any(), what
    assert np.all(got[ref == 0] == 0), what
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = np.broadcast_to(bound, err.shape)
    worst = int(np.argmax(err - bound)) if err.size else 0
    assert np.all(err <= bound), (what, got[worst], ref[worst], err[worst], bound[worst])
    return differ


def _local_references(A, links):
    """{name: (fp32 restatement, bound)}: RA with 1 ulp + 1e-13·Σ|term|, Jaccard and PA with 1 ulp"""
    ra, mag = M.ra(A, links, with_magnitude=True)
    jac, pa = M.jaccard(A, links), M.pa(A, links)
    return {"ra": (ra, M.ulp32(ra) + 1e-13 * mag), "jaccard": (jac, M.ulp32(jac)), "pa": (pa, M.ulp32(pa))}


def _both_orders(links):
    return (("(s, d)", links), ("(d, s)", links[::-1].copy()))


def _katz_abi(h, sources, links, beta=0.005, max_len=3, width=0):
    """s3grl_heuristics_katz as the C ABI has it: `sources` in the given order -> scores [L]"""
    from s3grl_amd import _native as N

    dev = h.engine.device
    s_d = torch.as_tensor(np.asarray(sources, dtype=np.int32)).to(dev)
    l_d = torch.as_tensor(np.ascontiguousarray(links, dtype=np.int32)).to(dev)
    out = torch.full((links.shape[1],), float("nan"), dtype=torch.float32, device=dev)
    N.check(N.lib().s3grl_heuristics_katz(h._h, N.ptr(s_d), len(sources), N.ptr(l_d), links.shape[1], float(beta),
                                          int(max_len), int(width), N.ptr(out)), "s3grl_heuristics_katz")
    return _np(out)


# ---- local indices ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("values", VALUE_SETS)
def test_local_indices_on_the_comb(values):
    """Row lengths 0, 1, 2, 63, 64, 65, 127, 128, 129 and 200 in every pairing, every overlap pattern in both
    directions, s == d.  A_int: Jaccard and PA bit-equal.  A_signed: columns of sum 0 (weight 0: they contribute
    nothing), 1, 0.5 and -2 (finite weights, kept); no NaN anywhere."""
    c = K.comb_graph()
    A = getattr(c, values)
    h = _heur(A)
    for name, links in _both_orders(c.links):
        for index, (ref, bound) in _local_references(A, links).items():
            got = _np(getattr(h, index)(links))
            _assert_within(f"{index} {values} {name}", got, ref, bound)
            if values == "A_int" and index != "ra":
                assert np.array_equal(_bits(got), _bits(ref)), (index, name)
        assert np.array_equal(_bits(_np(h.jaccard(links))), _bits(M.jaccard(A, links))), name   # structural: exact
    if values == "A_signed":
        zero = np.zeros(A.shape[0], dtype=bool)
        zero[c.columns["zero"]] = True
        common = [np.intersect1d(c.rows[s], c.rows[d]) for s, d in c.links.T]
        only_zero = np.array([len(k) > 0 and zero[k].all() for k in common])
        some_zero = np.array([zero[k].any() for k in common])
        assert some_zero.sum() >= 10
        got = _np(h.ra(c.links))
        assert np.all(got[only_zero] == 0) and np.isfinite(got).all()
    h.close()


@pytest.mark.parametrize("values", VALUE_SETS)
def test_short_link_lists_equal_the_long_one(values):
    """1, 3, 4 and 5 links: a partly filled last workgroup"""
    c = K.comb_graph()
    h = _heur(getattr(c, values))
    for fn in (h.ra, h.jaccard, h.pa):
        whole = _np(fn(c.links))
        for L, at in c.cuts.items():
            part = _np(fn(c.links[:, at]))
            assert part.shape == (L,) and _same_bits(part, whole[at]), (values, L)
        assert _same_bits(_np(fn(c.links[:, :1])), whole[:1])
    h.close()


def test_cn_and_aa_keep_their_bits_around_the_new_calls():
    c = K.comb_graph()
    for values in VALUE_SETS:
        A = getattr(c, values)
        h = _heur(A)
        before = [_np(h.cn(c.links)), _np(h.aa(c.links))]
        for fn in (h.ra, h.jaccard, h.pa, h.katz):
            fn(c.links)
        after = [_np(h.cn(c.links)), _np(h.aa(c.links))]
        h.close()
        for a, b in zip(before, after):
            assert _same_bits(a, b), values
        if values == "A_int":
            assert np.array_equal(_bits(before[0]), _bits(R.cn(A, c.links)))


@lru_cache(maxsize=None)
def _star_heur():
    return _heur(K.star(70000))


def test_star_pairs():
    """hub - leaf, leaf - leaf and hub - hub: a walked row of one entry against 70 000, and 70 000 against itself"""
    A, h = K.star(70000), _star_heur()
    links = np.array([[0, 1, 7, 70000, 0, 70000, 1], [0, 2, 70000, 1, 1, 0, 1]])
    ra, jac, pa = _np(h.ra(links)), _np(h.jaccard(links)), _np(h.pa(links))
    # every leaf column sums to 1 and the hub column to 70 000
    assert np.array_equal(ra[[0, 4, 5]], np.float32([70000, 0, 0]))
    assert np.all(np.abs(ra[[1, 2, 3, 6]].astype(np.float64) - 1 / 70000) <= M.ulp32(np.float32(1 / 70000)))
    assert np.array_equal(jac, np.float32([1, 1, 1, 1, 0, 0, 1]))
    assert np.array_equal(pa, np.float32([70000.0 ** 2, 1, 1, 1, 70000, 70000, 1]))
    for index, (ref, bound) in _local_references(A, links).items():
        _assert_within(f"{index} star", {"ra": ra, "jaccard": jac, "pa": pa}[index], ref, bound)


def test_empty_lists_and_the_kinds_of_the_c_abi():
    from s3grl_amd import _native as N

    c = K.comb_graph()
    h = _heur(c.A_float)
    e = np.zeros((2, 0), dtype=np.int64)
    for fn in (h.ra, h.jaccard, h.pa, h.katz):
        out = fn(e)
        assert out.shape == (0,) and out.is_cuda and out.dtype == torch.float32
    dev = h.engine.device
    links = torch.as_tensor(np.ascontiguousarray(c.links[:, :5], dtype=np.int32)).to(dev)
    out = torch.full((5,), float("nan"), dtype=torch.float32, device=dev)
    for kind in (-1, 5, 99):                                  # an unknown kind: refused, nothing written
        with pytest.raises(ValueError):
            N.check(N.lib().s3grl_heuristics_pairs(h._h, kind, N.ptr(links), 5, N.ptr(out)), "pairs")
        assert torch.isnan(out).all()
    for kind, fn in ((0, h.cn), (1, h.aa), (2, h.ra), (3, h.jaccard), (4, h.pa)):
        N.check(N.lib().s3grl_heuristics_pairs(h._h, kind, N.ptr(links), 5, N.ptr(out)), "pairs")
        assert _same_bits(_np(out), _np(fn(c.links[:, :5]))), kind
    with pytest.raises(ValueError):
        h.ra(np.array([[0], [c.A_float.shape[0]]]))
    with pytest.raises(ValueError):
        _katz_abi(h, [0, 1, 0], c.links[:, :1] * 0)            # a duplicate source
    with pytest.raises(ValueError):
        _katz_abi(h, [1], np.array([[0], [1]]))                # a link whose source is not listed
    with pytest.raises(ValueError):
        _katz_abi(h, [0], np.array([[0], [1]]), max_len=65)
    with pytest.raises(ValueError):
        _katz_abi(h, [0], np.array([[0], [1]]), beta=float("inf"))
    with pytest.raises(ValueError):
        _katz_abi(h, [0], np.array([[0], [1]]), width=96)
    ok = _katz_abi(h, [0], np.array([[0], [1]]))               # the object still works after a refusal
    assert _same_bits(ok, _np(h.katz(np.array([[0], [1]]))))
    h.close()
    from s3grl_amd import heuristics as H

    for twin, ref in ((H.RA, M.ra), (H.Jaccard, M.jaccard), (H.PA, M.pa), (H.Katz, M.katz)):
        s, ei = twin(c.A_float, torch.as_tensor(c.links))
        assert s.device.type == "cpu" and s.dtype == torch.float32 and torch.equal(ei, torch.as_tensor(c.links))
        assert np.max(np.abs(s.numpy() - ref(c.A_float, c.links)) / M.ulp32(ref(c.A_float, c.links))) <= 1


# ---- Katz -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", K.SINK_NS)
def test_katz_on_the_sink_graphs(n):
    """Sources: sinks with and without in-edges, nodes without in-edges, in-rows of 0..9 entries; every source paired
    with itself."""
    g, src, links = _sink_case(n)
    if n > 1:
        assert np.isin(src, g.sinks).any() and np.isin(src, g.orphans).any()
    assert np.all(np.isin(src, links[0][links[0] == links[1]]))
    h = _heur(g.A)
    differ = total = 0
    for max_len in MAX_LENS:
        for beta in BETAS:
            ref = M.katz(g.A, links, beta, max_len)
            got = _np(h.katz(links, beta=beta, max_len=max_len))
            differ += _assert_within(f"Katz n={n} beta={beta} max_len={max_len}", got, ref,
                                     M.katz_bound(g.A, links, beta, max_len))
            total += ref.size
    print(f"[heuristics more] Katz n={n}, all {len(MAX_LENS) * len(BETAS)} runs: {differ} of {total} not bit-equal")
    h.close()


def test_katz_on_the_integer_comb_is_exact():
    """Integer weights and a dyadic β: every sum is exact in fp64, so the scores are the restatement's bits"""
    c = K.comb_graph()
    h = _heur(c.A_int)
    for max_len in (3, 4, 7):
        ref = M.katz(c.A_int, c.links, 0.5, max_len)
        got = _np(h.katz(c.links, beta=0.5, max_len=max_len))
        assert np.count_nonzero(ref) > 100 and np.array_equal(_bits(got), _bits(ref)), max_len
    h.close()


@pytest.mark.parametrize("values", ("A_float", "A_signed"))
def test_katz_on_the_float_and_signed_comb(values):
    c = K.comb_graph()
    A = getattr(c, values)
    h = _heur(A)
    for beta, max_len in ((0.005, 3), (0.5, 7), (-0.5, 4), (1.0, 2)):
        _assert_within(f"Katz {values} beta={beta} max_len={max_len}", _np(h.katz(c.links, beta=beta, max_len=max_len)),
                       M.katz(A, c.links, beta, max_len), M.katz_bound(A, c.links, beta, max_len))
    h.close()


@pytest.mark.parametrize("max_len", (3, 4))
def test_katz_bits_do_not_depend_on_count_width_or_order(max_len):
    """1, 63, 64, 65, 128 and 129 sources at widths 64, 128 and the default, in two source orders: each source has
    the bits it has when solved alone, and two runs are identical.  Through `Heuristics.katz` with duplicated links
    and sources: the same bits again."""
    g = K.sink_graph(1041)
    pool, dests = _layout_pool(g)
    kw = dict(beta=0.5, max_len=max_len)
    h = _heur(g.A)
    alone = {int(u): _bits(_katz_abi(h, [u], _links_to([u], dests), **kw)) for u in pool}
    ref = M.katz(g.A, _links_to(pool, dests), **kw)
    _assert_within(f"Katz alone max_len={max_len}", np.concatenate([alone[int(u)] for u in pool]).view(np.float32),
                   ref, M.katz_bound(g.A, _links_to(pool, dests), **kw))
    rng = np.random.default_rng(6)

    def check(sources, width, what):
        links = _links_to(sources, dests, rng)
        out = _katz_abi(h, sources, links, width=width, **kw)
        assert not np.isnan(out).any(), what
        assert np.array_equal(_bits(out), _bits(_katz_abi(h, sources, links, width=width, **kw))), what   # two runs
        for u in sources:
            mine = np.nonzero(links[0] == u)[0]
            for b, dst in zip(alone[int(u)], np.r_[u, dests]):   # the order `alone` is in
                at = mine[links[1][mine] == dst]
                assert len(at) and np.all(_bits(out[at]) == b), (what, int(u), int(dst))

    for count in (1, 63, 64, 65, 128, 129):
        for width in (64, 128, 0):
            for sources in (pool[:count], np.sort(pool[:count])[::-1]):
                check(sources, width, (count, width))
    check(pool[3:129], 64, "another start")
    # the Python entry: sources repeated across links, links duplicated, in a shuffled order
    links = _links_to(pool, dests)
    links = np.concatenate([links, links[:, ::5]], axis=1)[:, rng.permutation(links.shape[1] + len(links[0][::5]))]
    for width in (0, 64):
        got = _np(h.katz(links, block_width=width, **kw))
        for u in pool[::9]:
            for b, dst in zip(alone[int(u)], np.r_[u, dests]):
                at = (links[0] == u) & (links[1] == dst)
                assert at.any() and np.all(_bits(got[at]) == b), (width, int(u), int(dst))
    h.close()


def test_katz_on_the_star():
    """Hub and leaf sources at max_len 4: the hub's column has 70 000 entries, so m = 70 000 in the bound"""
    A, h = K.star(70000), _star_heur()
    links = np.array([[0, 0, 0, 1, 1, 1, 1, 70000, 70000], [0, 1, 70000, 0, 1, 2, 70000, 0, 70000]])
    assert M.max_column_entries(A) == 70000
    for beta in (0.005, 0.5):
        ref = M.katz(A, links, beta, 4)
        got = _np(h.katz(links, beta=beta, max_len=4))
        _assert_within(f"Katz star beta={beta}", got, ref, M.katz_bound(A, links, beta, 4))
        # hub -> hub: β²·70000 + β⁴·70000²; leaf -> another leaf: β² + β⁴·70000
        assert np.isclose(got[0], beta ** 2 * 7e4 + beta ** 4 * 4.9e9, rtol=1e-6)
        assert np.isclose(got[5], beta ** 2 + beta ** 4 * 7e4, rtol=1e-6)


def test_katz_overflow_becomes_inf():
    """A score beyond fp32 becomes ±inf, as the conversion gives it"""
    A = K.star(9)
    h = _heur(A)
    links = np.array([[0, 0, 1, 1], [0, 1, 0, 2]])
    got = _np(h.katz(links, beta=-1e10, max_len=5))
    # hub -> hub and leaf -> leaf: even walks only, β⁴·81 and β⁴·9; hub -> leaf and back: odd walks only, β⁵·81
    assert np.array_equal(got, np.float32([np.inf, -np.inf, -np.inf, np.inf]))
    assert np.array_equal(got, M.katz(A, links, -1e10, 5))
    assert np.isfinite(_np(h.katz(links, beta=-1e10, max_len=3))).all()
    h.close()


# ---- end to end -------------------------------------------------------------------------------------------------

def test_run_heuristic_usair_matches_restatement():
    from s3grl_amd.heuristics import evaluate_auc, run_heuristic

    sp = _split("usair")
    lists = [sp.links["valid"][0], sp.links["valid"][1], sp.links["test"][0], sp.links["test"][1]]
    fns = {"RA": M.ra, "JACCARD": M.jaccard, "PA": M.pa, "KATZ": M.katz}
    for name, fn in fns.items():
        sc = [fn(sp.A, L) for L in lists]
        want = evaluate_auc(np.r_[sc[0], sc[1]], np.r_[np.ones(len(sc[0])), np.zeros(len(sc[1]))],
                            np.r_[sc[2], sc[3]], np.r_[np.ones(len(sc[2])), np.zeros(len(sc[3]))])
        got = run_heuristic(sp, name)
        for k in ("AUC", "AP"):
            assert np.allclose(got[k], want[k], rtol=0, atol=1e-6), (name, k, got[k], want[k])
        print(f"[heuristics more] USAir {name}: {got}")
    a = run_heuristic(sp, "katz", beta=0.05, max_len=5)        # the keyword arguments reach katz
    sc = [M.katz(sp.A, L, 0.05, 5) for L in lists]
    want = evaluate_auc(np.r_[sc[0], sc[1]], np.r_[np.ones(len(sc[0])), np.zeros(len(sc[1]))],
                        np.r_[sc[2], sc[3]], np.r_[np.ones(len(sc[2])), np.zeros(len(sc[3]))])
    assert np.allclose(a["AUC"], want["AUC"], rtol=0, atol=1e-6) and a != run_heuristic(sp, "KATZ")


@pytest.mark.parametrize("kind", ("KATZ", "RA"))
def test_recommend_on_cora(kind):
    """recommend's top-10 of 64 sources equals the segment top-K of the restatement's scores over `candidates`.  A tie
    can be moved by a last-bit difference: the score vectors are compared within the bound, the node ids only where
    the k-th and (k+1)-th restated scores differ by more than twice the bound."""
    import recommend_reference as ref
    from s3grl_amd import recommend as Rc
    from s3grl_amd.engine import default_engine
    from s3grl_amd.heuristics import Heuristics

    eng = default_engine("cuda:0")
    A = _split("cora").A
    G, h = eng.graph(A), Heuristics(A, device="cuda:0")
    n, k = A.shape[0], 10
    sources = np.random.default_rng(9).choice(n, 64, replace=False)
    top = Rc.recommend(G, sources, Rc.HeuristicScorer(h, kind), k=k, hops=2)
    seg_ptr, cand = Rc.candidates(G, sources, 2)
    seg_ptr, cand = seg_ptr.cpu().numpy(), cand.cpu().numpy()
    pairs = np.stack([np.repeat(sources, np.diff(seg_ptr)), cand.astype(np.int64)])
    if kind == "KATZ":
        scores, bound = M.katz(A, pairs), M.katz_bound(A, pairs, 0.005, 3)
    else:
        scores, mag = M.ra(A, pairs, with_magnitude=True)
        bound = M.ulp32(scores) + 1e-13 * mag
    nodes, vals, count = ref.segment_topk(scores, seg_ptr, cand, k)
    got_nodes, got_vals = top.nodes.cpu().numpy(), top.scores.cpu().numpy()
    assert np.array_equal(top.count.cpu().numpy(), count) and count.max() == k
    compared = 0
    for i in range(len(sources)):
        a, b, m = int(seg_ptr[i]), int(seg_ptr[i + 1]), int(count[i])
        tol = float(bound[a:b].max()) if b > a else 0.0
        assert np.all(np.abs(got_vals[i, :m].astype(np.float64) - vals[i, :m]) <= tol), (kind, i)
        assert np.all(got_nodes[i, m:] == -1)
        ranked = np.sort(scores[a:b].astype(np.float64))[::-1]
        if m == b - a or ranked[m - 1] - ranked[m] > 2 * tol:
            assert set(got_nodes[i, :m]) == set(nodes[i, :m]), (kind, i)
            compared += 1
    print(f"[heuristics more] recommend {kind} on Cora: node ids compared for {compared} of {len(sources)} sources, "
          f"{int(np.count_nonzero(got_nodes != nodes))} ids differ in position")
    assert compared >= 16
    G.close()
    h.close()
