"""The NCN kernels (csrc/s3grl_ncn.hip: cn_lists_kernel, segment_sum_kernel) against the numpy restatement
(tests/ncn_reference.py; tests/test_ncn_host.py checks it against the definitions and shows that its named faults
leave the comparison used here).

Every comparison is equality of bytes: the lists are integers, and the order of every fp32 addition is part of the
specification.  Calls through the C ABI fill their outputs with a sentinel first (-1, NaN), so an
entry the kernels fail to write cannot pass by holding a right answer from an earlier call's memory.  Values are
uniform in [-1, 1] with |x| >= 2^-20: no subnormal can arise, so flush-to-zero cannot explain a difference."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import ncn_cases as NC
import ncn_reference as R

pytestmark = pytest.mark.gpu


def _engine():
    from s3grl_amd.engine import default_engine

    return default_engine()


def _np(t):
    return t.detach().cpu().numpy()


def _same(what, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    differ = int(np.count_nonzero(got.view(np.uint8).reshape(-1) != ref.view(np.uint8).reshape(-1))) if got.size else 0
    print(f"[ncn] {what}: {differ} of {got.nbytes} bytes unequal to the restatement")
    assert differ == 0, what


def _graph(A):
    from s3grl_amd.heuristics import canonical_csr

    A = canonical_csr(A)
    dev = _engine().device
    return (torch.as_tensor(A.indptr.astype(np.int64)).to(dev), torch.as_tensor(A.indices.astype(np.int32)).to(dev),
            A.shape[0])


GUARD = 16


def _abi_lists(A, links, flag):
    """s3grl_cn_count and s3grl_cn_fill into arrays of -1 -> (ptr int64 [L+1], idx int32) as numpy; the GUARD entries
    past the end of idx must stay untouched."""
    from s3grl_amd import _native as N

    eng = _engine()
    ip, ix, n = _graph(A)
    links = np.asarray(links, dtype=np.int64).reshape(2, -1)
    L = links.shape[1]
    l_d = torch.as_tensor(links.astype(np.int32)).to(eng.device).contiguous()
    cnt = torch.full((L,), -1, dtype=torch.int64, device=eng.device)
    N.check(N.lib().s3grl_cn_count(eng._ctx, n, N.ptr(ip), N.ptr(ix), ix.numel(), N.ptr(l_d), L, int(flag),
                                   N.ptr(cnt)), "s3grl_cn_count")
    ptr = torch.zeros(L + 1, dtype=torch.int64, device=eng.device)
    ptr[1:] = torch.cumsum(cnt, 0)
    total = int(ptr[-1])
    assert 0 <= total <= ix.numel() * max(L, 1)
    idx = torch.full((total + GUARD,), -1, dtype=torch.int32, device=eng.device)
    N.check(N.lib().s3grl_cn_fill(eng._ctx, n, N.ptr(ip), N.ptr(ix), ix.numel(), N.ptr(l_d), L, int(flag),
                                  N.ptr(ptr), total, N.ptr(idx)), "s3grl_cn_fill")
    torch.cuda.synchronize()
    assert bool((idx[total:] == -1).all()), "the fill wrote past the end of the lists"
    return _np(ptr), _np(idx[:total])


def _abi_sum(h, ptr, idx):
    """s3grl_segment_sum of a device h (as given: aligned or not) into an array of NaN -> numpy fp32 [R, H]"""
    from s3grl_amd import _native as N

    eng = _engine()
    R_ = len(ptr) - 1
    p_d = torch.as_tensor(np.asarray(ptr, dtype=np.int64)).to(eng.device)
    i_d = torch.as_tensor(np.asarray(idx, dtype=np.int32)).to(eng.device)
    out = torch.full((R_, h.shape[1]), float("nan"), dtype=torch.float32, device=eng.device)
    N.check(N.lib().s3grl_segment_sum(eng._ctx, N.ptr(h), h.shape[0], h.shape[1], N.ptr(p_d), N.ptr(i_d), R_,
                                      N.ptr(out)), "s3grl_segment_sum")
    torch.cuda.synchronize()
    return _np(out)


# ---- the lists ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", (0, 1))
@pytest.mark.parametrize("name", ("lengths", "hub", "directed", "random"))
def test_lists_equal_the_restatement(name, flag):
    A, links = NC.list_cases()[name]
    ref_ptr, ref_idx = R.cn_lists(A, links, bool(flag))
    ptr, idx = _abi_lists(A, links, flag)
    _same(f"{name} flag {flag} ptr", ptr, ref_ptr)
    _same(f"{name} flag {flag} idx", idx, ref_idx)
    rev_ptr, rev_idx = _abi_lists(A, links[::-1].copy(), flag)           # both link orders: the lists are equal
    _same(f"{name} flag {flag} reversed ptr", rev_ptr, ref_ptr)
    _same(f"{name} flag {flag} reversed idx", rev_idx, ref_idx)


@pytest.mark.parametrize("size", NC.LIST_SIZES)
def test_link_lists_of_few_links_beside_a_long_row(size):
    A, links = NC.prefix_links(size)
    for flag in (0, 1):
        ref_ptr, ref_idx = R.cn_lists(A, links, bool(flag))
        ptr, idx = _abi_lists(A, links, flag)
        _same(f"{size} links flag {flag} ptr", ptr, ref_ptr)
        _same(f"{size} links flag {flag} idx", idx, ref_idx)


def test_bad_ids_are_refused_before_any_launch():
    from s3grl_amd import ncn

    A, _ = NC.hub_case()
    for bad in ([[0, 900], [1, 0]], [[0, -1], [1, 2]], [[0, 1], [1, 1 << 20]]):
        with pytest.raises(ValueError):
            _abi_lists(A, np.array(bad), 1)
        with pytest.raises(ValueError):
            ncn.CommonNeighbours(A, np.array(bad))
        with pytest.raises(ValueError):
            ncn.CommonNeighbours(_graph(A), torch.as_tensor(np.array(bad)).to(_engine().device))
    with pytest.raises(ValueError):
        ncn.CommonNeighbours(A, np.array([[0, 1, 2]]))
    ip, ix, n = _graph(A)
    with pytest.raises(ValueError, match="malformed"):
        ncn.CommonNeighbours((ip, ix + 1, n), np.array([[0], [1]]))         # a column == N
    with pytest.raises(ValueError, match="malformed"):
        ncn.CommonNeighbours((ip.flip(0), ix, n), np.array([[0], [1]]))


def test_the_object_equals_the_abi_on_a_matrix_and_on_a_device_triple():
    from s3grl_amd import ncn
    from s3grl_amd.heuristics import Heuristics

    A, links = NC.list_cases()["random"]
    for flag in (True, False):
        ref_ptr, ref_idx = R.cn_lists(A, links, flag)
        for graph, ll in ((A, links), (_graph(A), torch.as_tensor(links).to(_engine().device)), (A, torch.as_tensor(links))):
            cn = ncn.CommonNeighbours(graph, ll, exclude_endpoints=flag)
            assert cn.ptr.is_cuda and cn.idx.is_cuda and cn.counts.is_cuda and len(cn) == links.shape[1]
            _same("object ptr", _np(cn.ptr), ref_ptr)
            _same("object idx", _np(cn.idx), ref_idx)
            _same("object counts", _np(cn.counts), np.diff(ref_ptr))
            t_ptr, t_link = R.transpose(ref_ptr, ref_idx, A.shape[0])
            _same("object t_ptr", _np(cn.t_ptr), t_ptr)
            _same("object t_link", _np(cn.t_link), t_link)
    assert A.diagonal().sum() == 0
    h = Heuristics(A)
    try:
        _same("counts against Heuristics.cn", _np(cn.counts).astype(np.float32), _np(h.cn(links)))
    finally:
        h.close()
    empty = ncn.CommonNeighbours(A, np.zeros((2, 0), dtype=np.int64))
    assert tuple(empty.ptr.shape) == (1,) and empty.idx.numel() == 0 and empty.t_link.numel() == 0


# ---- the segment sum ------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _segment_reference(H):
    M, ptr, idx = NC.segment_case()
    h = R.values((M, H), seed=H)
    return h, R.segment_sum(h, ptr, idx)


@pytest.mark.parametrize("H", NC.WIDTHS)
def test_segment_sum_equals_the_restatement_at_every_length_and_width(H):
    M, ptr, idx = NC.segment_case()
    h, ref = _segment_reference(H)
    h_d = torch.as_tensor(h).to(_engine().device)
    assert h_d.data_ptr() % 16 == 0
    got = _abi_sum(h_d, ptr, idx)
    _same(f"segment sum H {H}", got, ref)
    _same(f"segment sum H {H}, second call", _abi_sum(h_d, ptr, idx), got)
    for R_ in (0, 1, 5):
        p, i = NC.first_rows(ptr, idx, R_)
        _same(f"segment sum H {H}, R {R_}", _abi_sum(h_d, p, i), ref[:R_])
    p, i = ptr[3:5] - ptr[3], idx[ptr[3]:ptr[4]]                            # R = 1 with a short row
    _same(f"segment sum H {H}, one short row", _abi_sum(h_d, p, i), ref[3:4])


@pytest.mark.parametrize("H", (4, 32, 256, 260))
def test_segment_sum_on_a_misaligned_view_takes_the_scalar_path(H):
    M, ptr, idx = NC.segment_case()
    h, ref = _segment_reference(H)
    flat = torch.zeros(M * H + 1, dtype=torch.float32, device=_engine().device)
    view = flat[1:].view(M, H)
    view.copy_(torch.as_tensor(h))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    _same(f"misaligned H {H}", _abi_sum(view, ptr, idx), ref)


def test_segment_sum_keeps_negative_zero_and_gives_plus_zero_for_an_empty_row():
    h = R.values((8, 4), seed=0)
    h[3] = -0.0
    ptr, idx = np.array([0, 1, 3, 3, 4], np.int64), np.array([3, 3, 3, 2], np.int32)
    ref = R.segment_sum(h, ptr, idx)
    assert np.signbit(ref[0]).all() and np.signbit(ref[1]).all() and not np.signbit(ref[2]).any()
    _same("signed zeros", _abi_sum(torch.as_tensor(h).to(_engine().device), ptr, idx), ref)


def test_segment_sum_checks_its_lists_on_the_device():
    from s3grl_amd import ncn

    M, ptr, idx = NC.segment_case()
    dev = _engine().device
    h, ref = _segment_reference(5)
    h_d, p_d, i_d = torch.as_tensor(h).to(dev), torch.as_tensor(ptr).to(dev), torch.as_tensor(idx).to(dev)
    _same("python segment_sum", _np(ncn.segment_sum(h_d, p_d, i_d)), ref)
    bad = i_d.clone()
    bad[17] = M
    for p, i in ((p_d, bad), (p_d.flip(0), i_d), (p_d[:-1], i_d), (p_d + 1, i_d)):
        with pytest.raises(ValueError, match="malformed"):
            ncn.segment_sum(h_d, p, i)
    with pytest.raises(ValueError):
        ncn.segment_sum(h_d.double(), p_d, i_d)


# ---- autograd -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H", (5, 64))
def test_common_neighbour_sum_and_its_gradient(H):
    """Forward and z.grad equal the restatement to the bit, and both lie within (n - 1)·2^-24·Σ|terms| per entry of
    the fp64 dense [L, N] mask product: the first-order bound of ANY order of n - 1 fp32 additions of n terms."""
    from s3grl_amd import ncn

    A, links = NC.autograd_case()
    n, L = A.shape[0], links.shape[1]
    ptr, idx = R.cn_lists(A, links, True)
    z, g = R.values((n, H), seed=10 + H), R.values((L, H), seed=20 + H)
    dev = _engine().device
    cn = ncn.CommonNeighbours(A, links)
    z_d = torch.as_tensor(z).to(dev).requires_grad_(True)
    C = ncn.common_neighbour_sum(z_d, cn)
    C.backward(torch.as_tensor(g).to(dev))
    fwd, grad = _np(C), _np(z_d.grad)
    _same(f"forward H {H}", fwd, R.cn_sum(z, ptr, idx))
    _same(f"gradient H {H}", grad, R.cn_sum_grad(g, ptr, idx, n))
    mask = np.zeros((L, n))
    mask[np.repeat(np.arange(L), np.diff(ptr)), idx] = 1.0
    z64, g64 = z.astype(np.float64), g.astype(np.float64)
    for what, got, exact, terms, sums in (
            ("forward", fwd, mask @ z64, mask.sum(1, keepdims=True), mask @ np.abs(z64)),
            ("gradient", grad, mask.T @ g64, mask.sum(0)[:, None], mask.T @ np.abs(g64))):
        bound = np.maximum(terms - 1, 0) * 2.0 ** -24 * sums
        err = np.abs(got.astype(np.float64) - exact)
        print(f"[ncn] {what} H {H}: max error {err.max():.3e}, smallest slack {np.min(bound - err):.3e}")
        assert np.all(err <= bound), what
    held = mask.sum(0)[list(NC.HUBS)].tolist()
    assert held == [325, 65, 64, 1, 0] and not grad[NC.HUBS[4]].any()
    z2 = torch.as_tensor(z).to(dev).requires_grad_(True)                   # two runs are bit-identical
    C2 = ncn.common_neighbour_sum(z2, ncn.CommonNeighbours(A, links))
    C2.backward(torch.as_tensor(g).to(dev))
    assert torch.equal(C2, C) and torch.equal(z2.grad, z_d.grad)
    rows = ncn.endpoint_rows(z2, cn.links[0])
    assert torch.equal(rows, z2.detach()[cn.links[0].long()])
    with pytest.raises(ValueError):
        ncn.common_neighbour_sum(z2[:-1], cn)
    with pytest.raises(ValueError):
        ncn.common_neighbour_sum(z2.double(), cn)


# ---- end to end -----------------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def _usair():
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    return W.edge_split(n, e, seed=0)


def test_run_ncn_on_usair_learns_beats_chance_and_repeats():
    """The packaged USAir topology, no features, 8 epochs at hidden 64: every step's loss finite, the last epoch's
    mean below the first's, val and test AUC above 0.5 (chance), and two runs with one seed identical.  The values
    themselves are only printed."""
    from s3grl_amd import ncn

    split = _usair()
    history = []
    res = ncn.run_ncn(split, epochs=8, hidden=64, seed=1, history=history)
    steps = len(history) // 8
    assert len(history) == 8 * steps and steps == -(-split.links["train"][0].shape[1] // 1024)
    assert np.all(np.isfinite(history))
    first, last = float(np.mean(history[:steps])), float(np.mean(history[-steps:]))
    print(f"[ncn] run_ncn USAir: loss {first:.4f} -> {last:.4f}, AUC val {res['AUC'][0]:.4f} test {res['AUC'][1]:.4f}, "
          f"AP val {res['AP'][0]:.4f} test {res['AP'][1]:.4f}")
    assert last < first
    assert res["AUC"][0] > 0.5 and res["AUC"][1] > 0.5
    assert set(res) == {"AUC", "AP"} and all(len(v) == 2 for v in res.values())
    again_history = []
    again = ncn.run_ncn(split, epochs=8, hidden=64, seed=1, history=again_history)
    assert again == res and again_history == history


@pytest.mark.parametrize("kwargs", (dict(mask=False), dict(use_cn=False), dict(mask=False, use_cn=False)))
def test_run_ncn_ablations_run(kwargs):
    from s3grl_amd import ncn

    history = []
    res = ncn.run_ncn(_usair(), epochs=2, hidden=64, seed=1, history=history, **kwargs)
    print(f"[ncn] run_ncn USAir {kwargs}, 2 epochs: AUC test {res['AUC'][1]:.4f}, AP test {res['AP'][1]:.4f}")
    assert np.all(np.isfinite(history)) and len(history)
    assert all(0.0 <= x <= 1.0 for v in res.values() for x in v)
