"""The CN / AA / PPR kernels (csrc/s3grl_heuristics.hip) at their layout and value edges, on the graphs of
tests/heuristics_cases.py (tests/test_heuristics_host.py asserts what those graphs hold) against the fp64
restatement (tests/heuristics_reference.py).

Bounds.  Kernel and restatement both add the same fp64 terms, in another order, and round to fp32 once: the two
fp64 sums differ by about 1e-15 relative, so the fp32 results are equal or adjacent, which is the 1-ulp bound used
throughout (`_ulp32`: the spacing of fp32 at the restatement's value).  Where terms cancel (the signed comb) the
reordering noise is relative to Σ|term|, not to the sum, and 1e-13·Σ|term| is added.  PPR is pinned by running a
chosen number of iterations (tol = 0, max_iter = k) on both sides, so no stop on `tol` blurs the comparison.  Every
comparison prints how many fp32 results are not bit-equal; that count is a report, not a threshold.

Calls through the C ABI fill `out` with NaN and `iterations` with -1 first: an entry the kernels fail to write
cannot pass by holding a right answer from an earlier call's memory."""
from functools import lru_cache

import numpy as np
import pytest
import scipy.sparse as ssp
import torch

import heuristics_cases as K
import heuristics_reference as R
from test_gpu_heuristics import _check_ppr

pytestmark = pytest.mark.gpu

VALUE_SETS = ("A_int", "A_float", "A_signed")


def _heur(A):
    from s3grl_amd.heuristics import Heuristics

    return Heuristics(A)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    """fp32 arrays equal bit for bit, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


def _ulp32(ref):
    return np.spacing(np.abs(np.asarray(ref, dtype=np.float32))).astype(np.float64)


def _report(what, got, ref):
    differ = int(np.count_nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref)))))
    print(f"[heuristics shapes] {what}: {differ} of {got.size} fp32 scores not bit-equal to the restatement")
    return differ


def _assert_close(what, got, ref, noise=None):
    """NaN and ±0 where the restatement has them (signbit included), elsewhere within 1 fp32 ulp (+ noise)"""
    assert got.dtype == np.float32 and got.shape == ref.shape
    differ = _report(what, got, ref)
    nan, zero = np.isnan(ref), ref == 0
    assert np.array_equal(np.isnan(got), nan), what
    assert np.all(got[zero] == 0) and np.array_equal(np.signbit(got[zero]), np.signbit(ref[zero])), what
    fin = ~nan
    err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64))
    bound = _ulp32(ref[fin]) + (0.0 if noise is None else noise[fin])
    worst = int(np.argmax(err - bound)) if err.size else 0
    assert np.all(err <= bound), (what, got[fin][worst], ref[fin][worst], err[worst], bound[worst])
    return differ


def _pair_reference(A, links, aa):
    """(the restatement's fp32 scores, Σ_k |a_sk · a_dk · w_k| per link from the restatement's own terms)"""
    A = R.canonical(A)
    with np.errstate(divide="ignore", invalid="ignore"):
        B = ssp.csr_matrix(A.multiply(R.aa_weights(A)[None, :])) if aa else A
        M = ssp.csr_matrix(A[links[0]].multiply(B[links[1]]))
        ref = np.asarray(M.sum(1)).ravel().astype(np.float32)
        mag = np.asarray(abs(M).sum(1)).ravel()
        assert _same_bits(ref, R.aa(A, links) if aa else R.cn(A, links))
    return ref, mag


def _ppr_abi(h, sources, links, p=0.85, tol=1e-7, max_iter=100, width=0):
    """s3grl_heuristics_ppr as the C ABI has it: `sources` in the given order -> (scores [L], iterations [S])"""
    from s3grl_amd import _native as N

    dev = h.engine.device
    s_d = torch.as_tensor(np.asarray(sources, dtype=np.int32)).to(dev)
    l_d = torch.as_tensor(np.ascontiguousarray(links, dtype=np.int32)).to(dev)
    out = torch.full((links.shape[1],), float("nan"), dtype=torch.float32, device=dev)
    its = torch.full((len(sources),), -1, dtype=torch.int32, device=dev)
    N.check(N.lib().s3grl_heuristics_ppr(h._h, N.ptr(s_d), len(sources), N.ptr(l_d), links.shape[1], float(p),
                                         float(tol), int(max_iter), int(width), N.ptr(out), N.ptr(its)),
            "s3grl_heuristics_ppr")
    return _np(out), _np(its)


# ---- pairs kernel ----------------------------------------------------------------------------------------------

def _both_orders(links):
    return (("(s, d)", links), ("(d, s)", links[::-1].copy()))


def test_cn_on_the_integer_comb_is_exact():
    c = K.comb_graph()
    h = _heur(c.A_int)
    for name, links in _both_orders(c.links):
        got = _np(h.cn(links))
        assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(R.cn(c.A_int, links))), name
        ref, _ = _pair_reference(c.A_int, links, True)
        _assert_close(f"AA integer comb {name}", _np(h.aa(links)), ref)
    h.close()


def test_cn_aa_on_the_float_comb_within_one_ulp():
    c = K.comb_graph()
    h = _heur(c.A_float)
    for name, links in _both_orders(c.links):
        for aa in (False, True):
            ref, _ = _pair_reference(c.A_float, links, aa)
            got = _np(h.aa(links) if aa else h.cn(links))
            _assert_close(f"{'AA' if aa else 'CN'} float comb {name}", got, ref)
    h.close()


def test_cn_aa_on_the_signed_comb():
    """±1 terms cancel, and the column sums of exactly 1, exactly 0, 0.5 and -2 give weights 0, -0.0, negative and
    NaN.  A NaN-weighted key anywhere in row d makes AA(s, d) NaN, as the reference's sparse product does."""
    c = K.comb_graph()
    h = _heur(c.A_signed)
    for name, links in _both_orders(c.links):
        for aa in (False, True):
            ref, mag = _pair_reference(c.A_signed, links, aa)
            got = _np(h.aa(links) if aa else h.cn(links))
            _assert_close(f"{'AA' if aa else 'CN'} signed comb {name}", got, ref, noise=1e-13 * mag)
    h.close()


@pytest.mark.parametrize("values", VALUE_SETS)
def test_short_link_lists_equal_the_long_one(values):
    c = K.comb_graph()
    h = _heur(getattr(c, values))
    for fn in (h.cn, h.aa):
        whole = _np(fn(c.links))
        for L, at in c.cuts.items():
            part = _np(fn(c.links[:, at]))
            assert part.shape == (L,) and _same_bits(part, whole[at]), (values, L)
        assert _same_bits(_np(fn(c.links[:, :1])), whole[:1])
    h.close()


@lru_cache(maxsize=None)
def _star_heur():
    return _heur(K.star(70000))


def test_star_pairs():
    h = _star_heur()
    links = np.array([[0, 1, 7, 70000, 0, 70000, 1], [0, 2, 70000, 1, 1, 0, 1]])
    cn, aa = _np(h.cn(links)), _np(h.aa(links))
    assert np.array_equal(cn, np.float32([70000, 1, 1, 1, 0, 0, 1]))
    leaf = np.float32(1.0 / np.log(70000.0))
    assert np.all(np.abs(aa[[1, 2, 3, 6]].astype(np.float64) - 1.0 / np.log(70000.0)) <= _ulp32(leaf))
    assert np.all(aa[[0, 4, 5]] == 0) and not np.signbit(aa[[0, 4, 5]]).any()   # every leaf column sums to 1
    _assert_close("AA star", aa, R.aa(K.star(70000), links))


# ---- PPR at a chosen iteration count ---------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _sink_case(n):
    g = K.sink_graph(n)
    src = K.sink_sources(g)
    extra = [int(g.sinks[0]), int(g.orphans[0])] if n > 1 else []
    links = K.links_of(src, n, extra=extra)
    links.setflags(write=False)
    return g, src, links


@lru_cache(maxsize=None)
def _fixed_reference(n, k, p):
    g, _, links = _sink_case(n)
    ref, its = R.ppr_scores(g.A, links, p=p, tol=0.0, max_iter=k)
    ref.setflags(write=False)
    its.setflags(write=False)
    return ref, its


FIXED_RUNS = [(k, 0.85) for k in K.FIXED_KS] + [(k, p) for k in (2, 9) for p in (0.0, 1.0)]


@pytest.mark.parametrize("n", K.SINK_NS)
def test_ppr_after_exactly_k_iterations(n):
    g, src, links = _sink_case(n)
    if n > 1:
        assert np.isin(src, g.sinks).any() and np.isin(src, g.orphans).any()
    h = _heur(g.A)
    differ = total = 0
    for k, p in FIXED_RUNS:
        got, its = h.ppr(links, p=p, tol=0.0, max_iter=k, return_iterations=True)
        ref, ref_its = _fixed_reference(n, k, p)
        assert np.array_equal(_np(its), ref_its), (n, k, p)
        if p == 0.85 and n > 1:
            assert np.all(ref_its[~np.isin(links[0], g.sinks)] == k)
        differ += _assert_close(f"PPR n={n} k={k} p={p}", _np(got), ref)
        total += ref.size
    print(f"[heuristics shapes] PPR n={n}, all {len(FIXED_RUNS)} runs: {differ} of {total} not bit-equal")
    h.close()


def test_ppr_on_the_star_after_five_iterations():
    A = K.star(70000)
    links = np.array([[0, 0, 0, 1, 1, 1, 1], [0, 1, 70000, 0, 1, 2, 70000]])
    got, its = _star_heur().ppr(links, tol=0.0, max_iter=5, return_iterations=True)
    ref, ref_its = R.ppr_scores(A, links, tol=0.0, max_iter=5)
    assert np.array_equal(_np(its), ref_its) and np.all(ref_its == 5)
    _assert_close("PPR star k=5", _np(got), ref)


def test_ppr_columns_that_freeze_at_different_iterations():
    """A coarse tol: the columns stop between 1 and 26 iterations, so most are frozen while others run on, across
    several of the host's checks.  A frozen column must keep the iterate it stopped at."""
    g, src, links = _sink_case(1041)
    h = _heur(g.A)
    got, its = h.ppr(links, tol=K.COARSE_TOL, return_iterations=True)
    got, its = _np(got), _np(its)
    ref, ref_its = R.ppr_scores(g.A, links, tol=K.COARSE_TOL)
    assert np.array_equal(its, ref_its) and ref_its.min() < 8 < ref_its.max()
    _assert_close("PPR coarse tol", got, ref)
    running = ~np.isin(links[0], g.sinks)
    stops = ref_its[running].min()
    for u in np.unique(links[0][running & (ref_its == stops)])[:3]:   # the first to stop, each alone
        mine = links[0] == u
        alone = _np(h.ppr(links[:, mine], tol=K.COARSE_TOL))
        assert np.array_equal(_bits(alone), _bits(got[mine])), u
    h.close()


# ---- block layout ----------------------------------------------------------------------------------------------

def _layout_pool(g, count=129):
    """`count` distinct sources of every kind in a fixed shuffled order, and the destinations scored for each"""
    rng = np.random.default_rng(5)
    rest = np.setdiff1d(np.arange(g.n), np.r_[g.sinks, g.orphans, g.designated])
    special = np.unique(np.r_[g.sinks[:10], g.orphans[:4], g.designated])
    pool = np.r_[special, rng.choice(rest, count - len(special), replace=False)]
    assert len(np.unique(pool)) == count
    dests = np.r_[g.sinks[:2], g.orphans[:1], g.designated[[4, 9]], rng.integers(0, g.n, 7)]
    return rng.permutation(pool), dests


def _links_to(sources, dests, rng=None):
    s = np.repeat(np.asarray(sources, dtype=np.int64), len(dests) + 1)
    d = np.concatenate([np.r_[u, dests] for u in sources])
    L = np.stack([s, d])
    return L if rng is None else L[:, rng.permutation(L.shape[1])]


def _solved_alone(h, sources, dests, **kw):
    """{source: (fp32 bits of its scores at itself and `dests`, iterations)}, each source in a call of its own"""
    alone = {}
    for u in sources:
        out, its = _ppr_abi(h, [u], _links_to([u], dests), **kw)
        alone[int(u)] = (_bits(out), int(its[0]))
    return alone


def _check_layout(h, alone, sources, dests, width, rng, what, **kw):
    links = _links_to(sources, dests, rng)
    out, its = _ppr_abi(h, sources, links, width=width, **kw)
    assert not np.isnan(out).any(), what
    for j, u in enumerate(sources):
        bits, it = alone[int(u)]
        assert its[j] == it, (what, int(u), int(its[j]), it)
        plain = _links_to([u], dests)[1]                   # the order `bits` is in
        mine = np.nonzero(links[0] == u)[0]
        for b, dst in zip(bits, plain):
            at = mine[links[1][mine] == dst]
            assert len(at) and np.all(_bits(out[at]) == b), (what, int(u), int(dst))


def test_ppr_bits_do_not_depend_on_count_width_or_order():
    g = K.sink_graph(1041)
    pool, dests = _layout_pool(g)
    kw = dict(tol=0.0, max_iter=9)
    h = _heur(g.A)
    alone = _solved_alone(h, pool, dests, **kw)
    its = np.array([alone[int(u)][1] for u in pool])
    assert set(its[~np.isin(pool, g.sinks)]) == {9} and set(its[np.isin(pool, g.sinks)]) == {1}
    rng = np.random.default_rng(6)
    for count in (1, 63, 64, 65, 128, 129):
        for width in (64, 128, 0):
            for sources in (pool[:count], np.sort(pool[:count])[::-1]):
                _check_layout(h, alone, sources, dests, width, rng, (count, width), **kw)
    _check_layout(h, alone, pool[3:129], dests, 64, rng, "another start", **kw)
    h.close()


def test_ppr_frozen_sink_at_the_last_column_of_a_group():
    """A sink source stops at iteration 1; the other 63 columns of its group, and a second group, run on to 9."""
    g = K.sink_graph(1041)
    pool, dests = _layout_pool(g)
    indeg = np.diff(g.A.tocsc().indptr)
    sink = int(g.sinks[indeg[g.sinks] > 0][0])
    others = pool[~np.isin(pool, g.sinks)]
    sources = np.r_[others[:63], sink, others[63:70]]
    kw = dict(tol=0.0, max_iter=9)
    h = _heur(g.A)
    alone = _solved_alone(h, sources, dests, **kw)
    assert alone[sink][1] == 1 and all(alone[int(u)][1] == 9 for u in sources if u != sink)
    assert sources[63] == sink
    for width in (64, 128):
        _check_layout(h, alone, sources, dests, width, None, ("sink at column 63", width), **kw)
    h.close()


# ---- converged runs on directed graphs -------------------------------------------------------------------------

def _converged(A, links, dense_sources):
    h = _heur(A)
    got, its = h.ppr(links, return_iterations=True)
    _check_ppr(A, links, _np(got), _np(its))
    few = links[:, np.isin(links[0], dense_sources)]
    assert few.shape[1] >= len(dense_sources)
    conv = _np(h.ppr(few, tol=1e-12, max_iter=10000))
    dense = {int(s): R.ppr_dense(A, int(s)) for s in dense_sources}
    ref = np.array([dense[int(s)][d] for s, d in few.T])
    np.testing.assert_allclose(conv, ref, rtol=1e-5, atol=1e-7)
    h.close()


def test_ppr_converged_on_the_sink_graph():
    g, src, links = _sink_case(1041)
    indeg = np.diff(g.A.tocsc().indptr)
    ordinary = src[~np.isin(src, np.r_[g.sinks, g.orphans])]
    pick = [int(g.sinks[indeg[g.sinks] > 0][0]), int(src[np.isin(src, g.orphans)][0]), int(g.designated[9])]
    _converged(g.A, links, np.unique(np.r_[pick, ordinary[:3]]))


def test_ppr_converged_on_the_float_comb():
    c = K.comb_graph()
    src = np.unique(c.links[0])
    empty = src[np.diff(c.A_float.indptr)[src] == 0]
    assert len(empty)                                      # a source with an empty row: a sink of the comb
    _converged(c.A_float, c.links, np.r_[empty[:1], src[[3, len(src) // 2, -1]]])


# ---- one object, many calls ------------------------------------------------------------------------------------

def test_one_object_reused_across_calls():
    g = K.sink_graph(1041)
    pool, dests = _layout_pool(g)
    big, small = _links_to(pool, dests), _links_to(pool[40:43], dests)
    pairs = K.links_of(pool[:60], g.n)
    calls = [("ppr", big, dict(tol=0.0, max_iter=9, block_width=128)),
             ("ppr", small, dict(tol=0.0, max_iter=9)),
             ("cn", pairs, {}),
             ("ppr", big[:, ::3], dict(p=0.5, max_iter=30)),
             ("aa", pairs, {}),
             ("ppr", big[:, ::3], dict(p=0.85, max_iter=30))]
    h = _heur(g.A)
    reused = [_np(getattr(h, name)(links, **kw)) for name, links, kw in calls]
    h.close()
    for (name, links, kw), got in zip(calls, reused):
        fresh = _heur(g.A)
        want = _np(getattr(fresh, name)(links, **kw))
        fresh.close()
        assert np.array_equal(_bits(got), _bits(want)), (name, kw)
    assert not np.array_equal(reused[3], reused[5])        # p reaches the coefficients


# ---- the C ABI -------------------------------------------------------------------------------------------------

def test_c_abi_sources_may_be_a_superset_in_any_order():
    g, src, links = _sink_case(1041)
    rng = np.random.default_rng(8)
    more = np.setdiff1d(np.arange(g.n), src)[::37][:20]    # sources that no link uses, sinks among them or not
    sources = rng.permutation(np.r_[src, more])
    assert not np.array_equal(sources, np.sort(sources)) and len(sources) <= 129
    h = _heur(g.A)
    for kw in (dict(tol=0.0, max_iter=9), dict()):
        out, its = _ppr_abi(h, sources, links, **kw)
        _, ref_its = R.ppr_batched(g.A, sources, **kw)
        assert np.array_equal(its, ref_its), kw
        want, _ = h.ppr(links, return_iterations=True, **kw)
        assert np.array_equal(_bits(out), _bits(_np(want))), kw
    with pytest.raises(ValueError):
        _ppr_abi(h, np.r_[sources, sources[5]], links)     # a duplicate source
    missing = sources[sources != links[0][0]]
    with pytest.raises(ValueError):
        _ppr_abi(h, missing, links)                        # a link whose source is not listed
    out, _ = _ppr_abi(h, sources, links, tol=0.0, max_iter=9)   # the object still works after a refusal
    assert np.array_equal(_bits(out), _bits(_np(h.ppr(links, tol=0.0, max_iter=9))))
    h.close()
