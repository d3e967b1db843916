"""The NCNC kernels (csrc/s3grl_ncn.hip: cn_split_kernel, segment_sum_kernel<., true>, segment_dot_kernel) against the
numpy restatement (tests/ncnc_reference.py; tests/test_ncnc_host.py checks it against the definitions and shows that
its named faults leave the comparison used here).

Every comparison is equality of bytes, into outputs filled with a sentinel first (-1 for integers, NaN for floats) and
with guard entries past the end that must stay untouched.  Values and weights are uniform in [-1, 1] with |x| >= 2^-20
(the weights also hold exact 0.0, -0.0 and 1.0): no subnormal can arise, so flush-to-zero cannot explain a difference."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import ncn_cases as NC
import ncn_reference as NR
import ncnc_reference as R
import sketch_mask_cases as MC
import test_gpu_ncn as TN

pytestmark = pytest.mark.gpu

GUARD = 16
_engine, _np, _graph = TN._engine, TN._np, TN._graph


def _same(what, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    differ = int(np.count_nonzero(got.view(np.uint8).reshape(-1) != ref.view(np.uint8).reshape(-1))) if got.size else 0
    print(f"[ncnc] {what}: {differ} of {got.nbytes} bytes unequal")
    assert differ == 0, what


def _dev(a, dtype=None):
    return torch.as_tensor(np.asarray(a, dtype=dtype)).to(_engine().device).contiguous()


# ---- cases ----------------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def section_graph():
    """Four rows of every length d of NC.LENGTHS: two equal prefixes of a pool (against a longer prefix every key is
    shared, against the twin both rows are), a random subset of the pool (some shared) and a row from a second pool
    (none shared).  Links: all ordered pairs of the 36 nodes, u == v too.  No row holds an endpoint."""
    rng = np.random.default_rng(27)
    n, pool, other = 1500, np.arange(40, 800), np.arange(800, 1500)
    rows = [[] for _ in range(n)]
    for k, d in enumerate(NC.LENGTHS):
        rows[k], rows[9 + k] = pool[:d].tolist(), pool[:d].tolist()
        rows[18 + k] = np.sort(rng.choice(pool[:700], d, replace=False)).tolist()
        rows[27 + k] = other[:d].tolist()
    A = MC._csr(rows, n)
    u, v = np.meshgrid(np.arange(36), np.arange(36), indexing="ij")
    return A, np.stack([u.reshape(-1), v.reshape(-1)]).astype(np.int64)


def _cases():
    return dict(NC.list_cases(), sections=section_graph())


def test_the_section_graph_holds_what_it_says():
    A, links = section_graph()
    deg = np.diff(A.indptr)
    counts = R.split_lists(A, links, True)[0]
    u, v = links
    for d in NC.LENGTHS:
        for mine, other, own in ((u, v, counts[1]), (v, u, counts[2])):       # as u's row and as v's row
            m = (deg[mine] == d) & (u != v)
            assert (m & (deg[other] == d)).any()                              # an equally long other row,
            assert (m & (deg[other] < d)).any() or d == 0                     # a shorter one
            assert (m & (deg[other] > d)).any() or d == 600                   # and a longer one
            if d:
                assert (m & (counts[0] == d) & (own == 0)).any()              # all shared: its own section empty
                assert (m & (counts[0] == 0) & (own == d)).any()              # none shared: S0 empty
            if d >= 2:
                assert (m & (counts[0] > 0) & (own > 0)).any()                # some shared
    assert ((counts[1] == 0) & (counts[2] == 0) & (counts[0] > 0) & (u != v)).any()
    assert ((counts[0] == 0) & (counts[1] > 0) & (counts[2] > 0)).any()


def _abi_split(A, links, flag):
    """s3grl_cn_split_count and s3grl_cn_split_fill into arrays of -1 -> (counts [3, L], ptr [L+1], idx, side) as
    numpy; the GUARD entries past the end of counts, idx and side must stay untouched."""
    from s3grl_amd import _native as N

    eng = _engine()
    ip, ix, n = _graph(A)
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    L = links.shape[1]
    l_d = _dev(links, np.int32)
    cnt = torch.full((3 * L + GUARD,), -1, dtype=torch.int64, device=eng.device)
    N.check(N.lib().s3grl_cn_split_count(eng._ctx, n, N.ptr(ip), N.ptr(ix), ix.numel(), N.ptr(l_d), L, int(flag),
                                         N.ptr(cnt)), "s3grl_cn_split_count")
    torch.cuda.synchronize()
    assert bool((cnt[3 * L:] == -1).all()), "the count wrote past its output"
    counts = cnt[:3 * L].view(3, L)
    assert bool((counts >= 0).all())
    ptr = torch.zeros(L + 1, dtype=torch.int64, device=eng.device)
    ptr[1:] = torch.cumsum(counts.sum(0), 0)
    total = int(ptr[-1])
    assert 0 <= total <= 2 * ix.numel() * max(L, 1)
    idx = torch.full((total + GUARD,), -1, dtype=torch.int32, device=eng.device)
    side = torch.full((total + GUARD,), -1, dtype=torch.int32, device=eng.device)
    N.check(N.lib().s3grl_cn_split_fill(eng._ctx, n, N.ptr(ip), N.ptr(ix), ix.numel(), N.ptr(l_d), L, int(flag),
                                        N.ptr(cnt), N.ptr(ptr), total, N.ptr(idx), N.ptr(side)), "s3grl_cn_split_fill")
    torch.cuda.synchronize()
    assert bool((idx[total:] == -1).all()) and bool((side[total:] == -1).all()), "the fill wrote past the lists"
    return _np(counts), _np(ptr), _np(idx[:total]), _np(side[:total])


def _check_split(what, A, links, flag):
    ref = R.split_lists(A, links, bool(flag))
    got = _abi_split(A, links, flag)
    for name, g, r in zip(("counts", "ptr", "idx", "side"), got, ref):
        _same(f"{what} flag {flag} {name}", g, r)
    counts, ptr, idx, side = got
    L = links.shape[1]
    start = np.repeat(ptr[:-1], np.diff(ptr))
    rank = np.arange(len(idx)) - start
    owner = np.repeat(np.arange(L), np.diff(ptr))
    expect = (rank >= counts[0][owner]).astype(np.int32) + (rank >= (counts[0] + counts[1])[owner]).astype(np.int32)
    _same(f"{what} flag {flag} side against counts", side, expect)
    cn_ptr, cn_idx = TN._abi_lists(A, links, flag)                      # S0: the bytes of s3grl_cn_fill
    _same(f"{what} flag {flag} S0 counts", counts[0], np.diff(cn_ptr))
    _same(f"{what} flag {flag} S0 against s3grl_cn_fill", idx[side == 0], cn_idx)


# ---- the split lists ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", (0, 1))
@pytest.mark.parametrize("name", ("sections", "lengths", "hub", "directed", "random"))
def test_split_lists_equal_the_restatement(name, flag):
    A, links = _cases()[name]
    _check_split(name, A, links, flag)
    _check_split(name + " reversed", A, links[::-1].copy(), flag)         # both link orders: S1 and S2 change places


@pytest.mark.parametrize("size", NC.LIST_SIZES)
def test_split_lists_of_few_links_beside_a_long_row(size):
    A, links = NC.prefix_links(size)
    for flag in (0, 1):
        _check_split(f"{size} links", A, links, flag)


def test_bad_ids_are_refused_and_the_object_equals_the_abi():
    from s3grl_amd import ncn

    A, _ = NC.hub_case()
    for bad in ([[0, 900], [1, 0]], [[0, -1], [1, 2]], [[0, 1], [1, 1 << 20]]):
        with pytest.raises(ValueError):
            _abi_split(A, np.array(bad), 1)
        with pytest.raises(ValueError):
            ncn.SplitNeighbours(A, np.array(bad))
    with pytest.raises(ValueError):
        ncn.SplitNeighbours(A, np.array([[0, 1, 2]]))
    A, links = NC.list_cases()["directed"]
    for flag in (True, False):
        counts, ptr, idx, side = R.split_lists(A, links, flag)
        at, pairs = R.inner_pairs(links, ptr, idx, side)
        for graph, ll in ((A, links), (_graph(A), _dev(links))):
            sn = ncn.SplitNeighbours(graph, ll, exclude_endpoints=flag)
            assert all(t.is_cuda for t in (sn.ptr, sn.idx, sn.side, sn.counts, sn.inner_at, sn.inner_links))
            assert len(sn) == links.shape[1]
            for name, g, r in (("counts", sn.counts, counts), ("ptr", sn.ptr, ptr), ("idx", sn.idx, idx),
                               ("side", sn.side, side), ("inner_at", sn.inner_at, at), ("inner_links", sn.inner_links, pairs)):
                _same(f"object {name}", _np(g), r)
            t_ptr, t_link = NR.transpose(ptr, idx, A.shape[0])
            _same("object t_ptr", _np(sn.t_ptr), t_ptr)
            _same("object t_link", _np(sn.t_link), t_link)
            _same("object t_perm", _np(sn.t_perm), np.argsort(idx, kind="stable"))
    empty = ncn.SplitNeighbours(A, np.zeros((2, 0), dtype=np.int64))
    assert tuple(empty.ptr.shape) == (1,) and empty.idx.numel() == 0 and tuple(empty.counts.shape) == (3, 0)
    assert empty.inner_at.numel() == 0 and tuple(empty.inner_links.shape) == (2, 0)


def test_sizes_out_of_range_are_refused_with_a_live_context():
    from s3grl_amd import _native as N

    eng = _engine()
    lib, E = N.lib(), N.ERR_INVALID_ARGUMENT
    one = torch.zeros(8, dtype=torch.int64, device=eng.device)
    p = N.ptr(one)
    for n, nnz, L, flag in ((0, 0, 1, 1), (1 << 31, 0, 1, 1), (3, -1, 1, 1), (3, 0, -1, 1), (3, 0, 1, 2)):
        assert lib.s3grl_cn_split_count(eng._ctx, n, p, p, nnz, p, L, flag, p) == E
        assert lib.s3grl_cn_split_fill(eng._ctx, n, p, p, nnz, p, L, flag, p, p, 0, p, p) == E
    assert lib.s3grl_cn_split_fill(eng._ctx, 3, p, p, 0, p, 1, 1, p, p, -1, p, p) == E
    assert lib.s3grl_cn_split_count(eng._ctx, 3, None, p, 0, p, 1, 1, p) == E
    for M, H, R_ in ((3, 0, 1), (3, 65537, 1), (3, 4, -1), (1 << 31, 4, 1), (3, 4, 1 << 31)):
        assert lib.s3grl_segment_wsum(eng._ctx, p, M, H, p, p, p, R_, p) == E
        assert lib.s3grl_segment_dot(eng._ctx, p, R_, p, M, H, p, p, p) == E
    assert lib.s3grl_segment_wsum(eng._ctx, p, 3, 4, None, p, p, 1, p) == E
    assert lib.s3grl_segment_wsum(eng._ctx, p, 3, 4, p, p, p, 1, None) == E
    assert lib.s3grl_segment_dot(eng._ctx, None, 1, p, 3, 4, p, p, p) == E
    assert lib.s3grl_segment_dot(eng._ctx, p, 1, p, 3, 4, None, p, p) == E


# ---- the weighted sum and the dot -----------------------------------------------------------------------------------

def _abi_wsum(h, ptr, idx, w):
    """s3grl_segment_wsum of a device h (as given: aligned or not) into an array of NaN -> numpy fp32 [R, H]"""
    from s3grl_amd import _native as N

    eng = _engine()
    R_, H = len(ptr) - 1, h.shape[1]
    p_d, i_d, w_d = _dev(ptr, np.int64), _dev(idx, np.int32), _dev(w, np.float32)
    out = torch.full((R_ * H + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    N.check(N.lib().s3grl_segment_wsum(eng._ctx, N.ptr(h), h.shape[0], H, N.ptr(p_d), N.ptr(i_d), N.ptr(w_d), R_,
                                       N.ptr(out)), "s3grl_segment_wsum")
    torch.cuda.synchronize()
    assert bool(out[R_ * H:].isnan().all()), "the sum wrote past its output"
    return _np(out[:R_ * H].view(R_, H))


def _abi_dot(g, h, ptr, idx):
    """s3grl_segment_dot of device g and h (as given) into an array of NaN -> numpy fp32 [len(idx)]"""
    from s3grl_amd import _native as N

    eng = _engine()
    R_, E = len(ptr) - 1, len(idx)
    p_d, i_d = _dev(ptr, np.int64), _dev(idx, np.int32)
    out = torch.full((E + GUARD,), float("nan"), dtype=torch.float32, device=eng.device)
    N.check(N.lib().s3grl_segment_dot(eng._ctx, N.ptr(g), R_, N.ptr(h), h.shape[0], h.shape[1], N.ptr(p_d), N.ptr(i_d),
                                      N.ptr(out)), "s3grl_segment_dot")
    torch.cuda.synchronize()
    assert bool(out[E:].isnan().all()), "the dot wrote past its output"
    return _np(out[:E])


@lru_cache(maxsize=None)
def _segment_reference(H):
    """(h, g, w, weighted sum, dot) of NC.segment_case at width H, computed once"""
    M, ptr, idx = NC.segment_case()
    h, g, w = R.values((M, H), seed=H), R.values((len(ptr) - 1, H), seed=1000 + H), R.weights(len(idx), seed=2000 + H)
    assert (w > 0).any() and (w < 0).any() and (w == 0).sum() == 2 and np.signbit(w[w == 0]).sum() == 1
    return h, g, w, R.segment_wsum(h, ptr, idx, w), R.segment_dot(g, h, ptr, idx)


def _misaligned(a):
    flat = torch.zeros(a.size + 1, dtype=torch.float32, device=_engine().device)
    view = flat[1:].view(*a.shape)
    view.copy_(torch.as_tensor(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("H", NC.WIDTHS)
def test_weighted_sum_equals_the_restatement_at_every_length_and_width(H):
    M, ptr, idx = NC.segment_case()
    h, _, w, ref, _ = _segment_reference(H)
    h_d = _dev(h)
    assert h_d.data_ptr() % 16 == 0
    got = _abi_wsum(h_d, ptr, idx, w)
    _same(f"weighted sum H {H}", got, ref)
    _same(f"weighted sum H {H}, second call", _abi_wsum(h_d, ptr, idx, w), got)
    for R_ in (0, 1, 5):
        p, i = NC.first_rows(ptr, idx, R_)
        _same(f"weighted sum H {H}, R {R_}", _abi_wsum(h_d, p, i, w[:len(i)]), ref[:R_])
    ones = np.ones(len(idx), np.float32)
    unit = _abi_wsum(h_d, ptr, idx, ones)
    _same(f"unit weights H {H} against s3grl_segment_sum", unit, TN._abi_sum(h_d, ptr, idx))
    _same(f"unit weights H {H} against the unweighted restatement", unit, NR.segment_sum(h, ptr, idx))


@pytest.mark.parametrize("H", NC.WIDTHS)
def test_dot_equals_the_restatement_at_every_length_and_width(H):
    M, ptr, idx = NC.segment_case()
    h, g, _, _, ref = _segment_reference(H)
    h_d, g_d = _dev(h), _dev(g)
    assert h_d.data_ptr() % 16 == 0 and g_d.data_ptr() % 16 == 0
    got = _abi_dot(g_d, h_d, ptr, idx)
    _same(f"dot H {H}", got, ref)
    _same(f"dot H {H}, second call", _abi_dot(g_d, h_d, ptr, idx), got)
    for R_ in (0, 1, 5):
        p, i = NC.first_rows(ptr, idx, R_)
        _same(f"dot H {H}, R {R_}", _abi_dot(g_d, h_d, p, i), ref[:len(i)])


@pytest.mark.parametrize("H", (4, 32, 256, 260))
def test_misaligned_views_take_the_scalar_path_and_give_the_same_bytes(H):
    M, ptr, idx = NC.segment_case()
    h, g, w, ref_sum, ref_dot = _segment_reference(H)
    h_m, g_m, h_d, g_d = _misaligned(h), _misaligned(g), _dev(h), _dev(g)
    _same(f"misaligned weighted sum H {H}", _abi_wsum(h_m, ptr, idx, w), ref_sum)
    _same(f"misaligned dot H {H}", _abi_dot(g_m, h_m, ptr, idx), ref_dot)
    _same(f"dot H {H}, g misaligned only", _abi_dot(g_m, h_d, ptr, idx), ref_dot)
    _same(f"dot H {H}, h misaligned only", _abi_dot(g_d, h_m, ptr, idx), ref_dot)
    _same(f"VEC against scalar, weighted sum H {H}", _abi_wsum(h_d, ptr, idx, w), _abi_wsum(h_m, ptr, idx, w))
    _same(f"VEC against scalar, dot H {H}", _abi_dot(g_d, h_d, ptr, idx), _abi_dot(g_m, h_m, ptr, idx))


def test_signed_zero_weights_and_empty_rows():
    h = np.abs(R.values((8, 4), seed=0))
    ptr, idx = np.array([0, 1, 3, 3, 4, 6], np.int64), np.array([3, 3, 2, 1, 5, 5], np.int32)
    w = np.array([-0.0, 0.0, -0.0, -1.0, -0.0, -0.0], np.float32)
    ref = R.segment_wsum(h, ptr, idx, w)
    assert np.signbit(ref[0]).all() and not np.signbit(ref[1]).any() and not np.signbit(ref[2]).any()
    assert np.signbit(ref[4]).all() and (ref[4] == 0).all()                  # -0.0 + -0.0 stays -0.0
    _same("signed zero weights", _abi_wsum(_dev(h), ptr, idx, w), ref)
    g = np.zeros((5, 4), np.float32)
    g[0], g[1] = -0.0, R.values((4,), seed=1)
    dots = R.segment_dot(g, h, ptr, idx)
    # slot 0's products are all -0.0, but the 63 slots without a column hold +0.0 and the tree adds them
    assert dots[0] == 0 and not np.signbit(dots[0]) and dots[1] != 0
    _same("signed zero dot", _abi_dot(_dev(g), _dev(h), ptr, idx), dots)
    g256, h256 = np.full((5, 256), -0.0, np.float32), np.abs(R.values((8, 256), seed=2))
    full = R.segment_dot(g256, h256, ptr, idx)                               # every slot holds -0.0: so does the dot
    assert np.signbit(full).all() and (full == 0).all()
    _same("signed zero dot at H 256", _abi_dot(_dev(g256), _dev(h256), ptr, idx), full)


# ---- autograd -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("common", "split"))
@pytest.mark.parametrize("H", (5, 64))
def test_completed_neighbour_sum_and_its_two_gradients(H, kind):
    """Forward, z.grad and weights.grad equal the restatement to the bit and lie within n·2^-24·Σ|terms| per entry of
    an fp64 evaluation: n roundings on the longest path of a sum of n rounded products, in any order.  `common`: the
    NCN lists, where nodes sit in the lists of 0, 1, 64, 65 and 325 links; `split`: the NCNC lists."""
    from s3grl_amd import ncn

    A, links = NC.autograd_case()
    n, L = A.shape[0], links.shape[1]
    if kind == "common":
        ptr, idx = NR.cn_lists(A, links, True)
        make = lambda: ncn.CommonNeighbours(A, links)                       # noqa: E731
    else:
        _, ptr, idx, _ = R.split_lists(A, links, True)
        make = lambda: ncn.SplitNeighbours(A, links)                        # noqa: E731
    z, g, w = R.values((n, H), seed=10 + H), R.values((L, H), seed=20 + H), R.weights(len(idx), seed=30 + H)
    dev = _engine().device

    def run():
        lists = make()
        z_d, w_d = _dev(z).requires_grad_(True), _dev(w).requires_grad_(True)
        C = ncn.completed_neighbour_sum(z_d, lists, w_d)
        C.backward(_dev(g))
        return lists, C.detach(), z_d.grad, w_d.grad

    lists, C, gz, gw = run()
    _same(f"{kind} lists", _np(lists.idx), idx)
    fwd, grad_z, grad_w = _np(C), _np(gz), _np(gw)
    _same(f"{kind} forward H {H}", fwd, R.segment_wsum(z, ptr, idx, w))
    _same(f"{kind} z.grad H {H}", grad_z, R.wsum_grad_z(g, ptr, idx, w, n))
    _same(f"{kind} weights.grad H {H}", grad_w, R.segment_dot(g, z, ptr, idx))
    owner = np.repeat(np.arange(L), np.diff(ptr))
    W, held = np.zeros((L, n)), np.zeros((L, n))
    W[owner, idx], held[owner, idx] = w.astype(np.float64), 1.0
    z64, g64 = z.astype(np.float64), g.astype(np.float64)
    terms = g64[owner] * z64[idx]
    for what, got, exact, count, sums in (
            ("forward", fwd, W @ z64, held.sum(1, keepdims=True), np.abs(W) @ np.abs(z64)),
            ("z.grad", grad_z, W.T @ g64, held.sum(0)[:, None], np.abs(W).T @ np.abs(g64)),
            ("weights.grad", grad_w, terms.sum(1), float(H), np.abs(terms).sum(1))):
        bound = count * 2.0 ** -24 * sums
        err = np.abs(got.astype(np.float64) - exact)
        print(f"[ncnc] {kind} {what} H {H}: max error {err.max():.3e}, smallest slack {np.min(bound - err):.3e}")
        assert np.all(err <= bound), what
    if kind == "common":
        assert held.sum(0)[list(NC.HUBS)].tolist() == [325, 65, 64, 1, 0] and not grad_z[NC.HUBS[4]].any()
    else:
        assert held.sum(0).max() == 325 and held.sum(1).max() > R.CHUNK
    _, C2, gz2, gw2 = run()                                                  # two runs are bit-identical
    assert torch.equal(C2, C) and torch.equal(gz2, gz) and torch.equal(gw2, gw)
    z_d, w_d = _dev(z), _dev(w)
    with pytest.raises(ValueError):
        ncn.completed_neighbour_sum(z_d[:-1], lists, w_d)
    with pytest.raises(ValueError):
        ncn.completed_neighbour_sum(z_d.double(), lists, w_d)
    with pytest.raises(ValueError):
        ncn.completed_neighbour_sum(z_d, lists, w_d[:-1])
    with pytest.raises(ValueError):
        ncn.completed_neighbour_sum(z_d, lists, w_d.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ncn.completed_neighbour_sum(z_d, lists, w_d.cpu())


def test_the_twin_completes_with_ncn_probabilities_and_passes_gradient_through_them():
    from s3grl_amd import ncn

    A, links = NC.list_cases()["random"]
    links = links[:, :32]
    dev = _engine().device
    model = ncn.NCNCTwin(A.shape[0], hidden=16, dropout=0.0, seed=2).to(dev).eval()
    z = _dev(R.values((A.shape[0], 16), seed=3)).requires_grad_(True)
    sn = ncn.SplitNeighbours(A, links)
    assert sn.inner_at.numel() > 0
    w = model.completion_weights(z, sn)
    inner = ncn.CommonNeighbours(sn.csr, sn.inner_links, True)
    p = torch.sigmoid(ncn.NCNTwin.forward(model, z, inner))
    assert torch.equal(w[sn.inner_at], p) and bool((w[sn.side == 0] == 1).all()) and w.numel() == sn.idx.numel()
    logits = model(z, sn)
    assert logits.shape == (32,) and bool(torch.isfinite(logits).all())
    logits.sum().backward()
    through = z.grad.clone()
    frozen = ncn.NCNCTwin(A.shape[0], hidden=16, dropout=0.0, seed=2, detach_completion=True).to(dev).eval()
    z2 = z.detach().clone().requires_grad_(True)
    logits2 = frozen(z2, sn)
    logits2.sum().backward()
    assert torch.equal(logits2, logits) and not torch.equal(z2.grad, through)


# ---- end to end -----------------------------------------------------------------------------------------------------

USAIR_TEST_AUC = 0.9143                         # measured on the MI355X at this shape (profiles/ncnc_probe.json)
USAIR_TEST_AUC_FLOOR = USAIR_TEST_AUC - 0.03    # the rows of DESIGN.md §26's table move by about a point: three times that


def test_run_ncnc_on_usair_learns_and_stays_above_its_floor():
    """The packaged USAir topology, no features, 8 epochs at hidden 64 (`run_ncn`'s GPU-test shape): every step's loss
    finite, the last epoch's mean below the first's, and test AUC above 0.8843, which is 0.03 below the 0.9143 measured
    on the MI355X.  `run_ncn`'s value at the same shape is printed beside it (0.9416 when this was written) and not
    compared: one seed cannot say which of the two is higher."""
    from s3grl_amd import ncn

    split = TN._usair()
    history = []
    res = ncn.run_ncnc(split, epochs=8, hidden=64, seed=1, history=history)
    steps = len(history) // 8
    assert len(history) == 8 * steps and steps == -(-split.links["train"][0].shape[1] // 1024)
    first, last = float(np.mean(history[:steps])), float(np.mean(history[-steps:]))
    other = ncn.run_ncn(split, epochs=8, hidden=64, seed=1)
    print(f"[ncnc] run_ncnc USAir: loss {first:.4f} -> {last:.4f}, AUC val {res['AUC'][0]:.4f} test {res['AUC'][1]:.4f}, "
          f"AP val {res['AP'][0]:.4f} test {res['AP'][1]:.4f}; run_ncn at the same shape: AUC test {other['AUC'][1]:.4f}, "
          f"AP test {other['AP'][1]:.4f} (printed, not compared: one seed)")
    assert np.all(np.isfinite(history))
    assert last < first
    assert set(res) == {"AUC", "AP"} and all(len(v) == 2 for v in res.values())
    assert res["AUC"][1] > USAIR_TEST_AUC_FLOOR
