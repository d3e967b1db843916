"""CPU checks of the NCN restatement (tests/ncn_reference.py): the lists against a dense mask and
against a rebuild without the link's own entries; the counts against the existing CN restatement; the named faults
against byte equality, each on a case built for it; the refusals that need no device; and the public surface of the
three new symbols."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import heuristics_reference as HR
import ncn_cases as NC
import ncn_reference as R

REPO = Path(__file__).resolve().parent.parent


def _differ(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return int(np.count_nonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)))


def _split(ptr, idx):
    return [idx[ptr[l]:ptr[l + 1]] for l in range(len(ptr) - 1)]


# ---- the cases hold what they say ---------------------------------------------------------------------------------

def test_the_cases_hold_what_they_say():
    A, links = NC.length_graph()
    deg = np.diff(A.indptr)
    u, v = links
    assert set(deg[u].tolist()) == set(NC.LENGTHS) and (u == v).any()
    ptr, idx = R.cn_lists(A, links, False)
    # walked row (the shorter) of every length against a longer and an equally long searched row
    for d in NC.LENGTHS:
        assert ((np.minimum(deg[u], deg[v]) == d) & (np.maximum(deg[u], deg[v]) > d)).any() or d == 600
        assert ((deg[u] == d) & (deg[v] == d) & (u != v)).any()
    # a prefix row walked against a longer prefix row: every position survives, the 64-key boundaries too
    at = np.nonzero((u == 7) & (v == 8))[0][0]
    assert deg[7] == 129 and ptr[at + 1] - ptr[at] >= 128
    at = np.nonzero((u == 8) & (v == 18))[0][0]
    kept = np.isin(A.indices[A.indptr[8]:A.indptr[9]], idx[ptr[at]:ptr[at + 1]])
    assert kept.any() and not kept.all()                           # a random row against it: some survive
    loops = A.diagonal() != 0
    assert (loops[u] & (u != v)).any() and (loops[v] & (u != v)).any() and (loops[u] & (u == v)).any()
    A, links = NC.hub_case()
    assert np.diff(A.indptr)[:3].tolist() == [600, 260, 0] and A[:, 2].nnz == 0 and (links == 2).any()
    assert (links[:, 0] == links[:, 2]).all()                       # a repeated link
    M, ptr, idx = NC.segment_case()
    assert set(NC.SEGMENTS) <= set(np.diff(ptr).tolist()) and (idx[ptr[-2]:] == 7).all() and ptr[-1] - ptr[-2] == 300
    A, links = NC.autograd_case()
    ptr, idx = R.cn_lists(A, links, True)
    held = np.bincount(idx, minlength=A.shape[0])
    assert held[list(NC.HUBS)].tolist() == [325, 65, 64, 1, 0] and links.shape[1] == 525
    assert np.diff(ptr).max() > R.CHUNK                             # a forward list of more than one chunk


# ---- the lists ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", (False, True))
@pytest.mark.parametrize("name", ("random", "directed", "hub", "lengths"))
def test_lists_equal_a_dense_mask(name, flag):
    A, links = NC.list_cases()[name]
    ptr, idx = R.cn_lists(A, links, flag)
    dense = NC.dense_lists(A, links, flag)
    assert idx.dtype == np.int32 and ptr.dtype == np.int64 and len(ptr) == links.shape[1] + 1
    for got, ref in zip(_split(ptr, idx), dense):
        assert np.array_equal(got, ref)
    assert all(np.all(np.diff(s) > 0) for s in _split(ptr, idx))    # ascending, distinct


@pytest.mark.parametrize("name", ("directed", "random", "lengths"))
def test_exclude_endpoints_equals_a_rebuild_without_the_links_own_entries(name):
    A, links = NC.list_cases()[name]
    if name == "lengths":                                           # the links at rows with loops and partners
        at = np.isin(links, (4, 14, 5, 6, 16, 8, 18)).all(axis=0)
        links = links[:, at]
    ptr, idx = R.cn_lists(A, links, True)
    loops = A.diagonal() != 0
    u, v = links
    assert (loops[u] & ~loops[v] & (u != v)).any() or name == "random"
    assert (~loops[u] & loops[v] & (u != v)).any() or name == "random"
    assert (u == v).any() or name == "random"
    changed = 0
    for l, (a, b) in enumerate(links.T.tolist()):
        # removing (u, v) and (v, u) removes v from N(u) and u from N(v): neither can be common any more.  u == v:
        # the rebuild drops the self-loop, which is all the flag drops
        _, i2 = R.cn_lists(NC.without_link(A, a, b), np.array([[a], [b]]), False)
        assert np.array_equal(idx[ptr[l]:ptr[l + 1]], i2), (a, b)
        _, i0 = R.cn_lists(A, np.array([[a], [b]]), False)
        changed += len(i0) != len(i2)
    assert changed or name == "random"


@pytest.mark.parametrize("name", ("random", "hub"))
def test_counts_equal_the_existing_cn_restatement_without_self_loops(name):
    A, links = NC.list_cases()[name]
    loops = A.diagonal() != 0
    links = links[:, ~loops[links[0]] & ~loops[links[1]]]
    assert links.shape[1] > 20
    for flag in (False, True):
        ptr, _ = R.cn_lists(A, links, flag)
        assert np.array_equal(np.diff(ptr).astype(np.float32), HR.cn(A, links))


def test_both_link_orders_give_equal_lists():
    for name, (A, links) in NC.list_cases().items():
        a, b = R.cn_lists(A, links, True), R.cn_lists(A, links[::-1].copy(), True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name


# ---- the order of the additions: the named faults leave byte equality ----------------------------------------------

def test_the_sum_is_the_dense_product_within_the_derived_bound():
    A, links = NC.autograd_case()
    ptr, idx = R.cn_lists(A, links, True)
    z = R.values((A.shape[0], 5), seed=1)
    got = R.cn_sum(z, ptr, idx).astype(np.float64)
    mask = np.zeros((links.shape[1], A.shape[0]))
    mask[np.repeat(np.arange(links.shape[1]), np.diff(ptr)), idx] = 1.0
    n = np.diff(ptr)[:, None]
    bound = np.maximum(n - 1, 0) * 2.0 ** -24 * (mask @ np.abs(z.astype(np.float64)))
    assert np.all(np.abs(got - mask @ z.astype(np.float64)) <= bound)


def test_fault_unchunked_moves_an_ulp_on_a_row_of_130_entries():
    h = R.values((200, 16), seed=130)
    ptr, idx = np.array([0, 130], np.int64), np.random.default_rng(130).integers(0, 200, 130).astype(np.int32)
    good, bad = R.segment_sum(h, ptr, idx), R.segment_sum(h, ptr, idx, fault="unchunked")
    print(f"[ncn] unchunked: {_differ(good, bad)} bytes differ on a row of 130 entries")
    assert _differ(good, bad) > 0 and np.allclose(good, bad, rtol=0, atol=1e-4)
    short = np.array([0, 64], np.int64)                     # one chunk: chunking changes nothing
    assert _differ(R.segment_sum(h, short, idx[:64]), R.segment_sum(h, short, idx[:64], fault="unchunked")) == 0


def test_fault_from_zero_loses_the_sign_of_a_negative_zero():
    h = R.values((8, 4), seed=0)
    h[3] = -0.0
    for ptr, idx in ((np.array([0, 1], np.int64), np.array([3], np.int32)),
                     (np.array([0, 2], np.int64), np.array([3, 3], np.int32))):
        good, bad = R.segment_sum(h, ptr, idx), R.segment_sum(h, ptr, idx, fault="from_zero")
        assert np.all(np.signbit(good)) and not np.any(np.signbit(bad)) and _differ(good, bad) > 0
    empty = R.segment_sum(h, np.array([0, 0], np.int64), np.zeros(0, np.int32))
    assert not np.any(np.signbit(empty)) and np.all(empty == 0)      # an empty row is +0.0


def test_fault_descending_links_moves_an_ulp_in_the_gradient():
    A, links = NC.autograd_case()
    ptr, idx = R.cn_lists(A, links, True)
    g = R.values((links.shape[1], 8), seed=2)
    n = A.shape[0]
    good, bad = R.cn_sum_grad(g, ptr, idx, n), R.cn_sum_grad(g, ptr, idx, n, fault="descending_links")
    rows = np.nonzero((good.view(np.uint32) != bad.view(np.uint32)).any(axis=1))[0]
    print(f"[ncn] descending_links: gradient rows {rows.tolist()[:8]} differ")
    assert len(rows) and set(rows.tolist()) & set(NC.HUBS[:3])
    t_ptr, t_link = R.transpose(ptr, idx, n)
    assert all(np.all(np.diff(t_link[t_ptr[w]:t_ptr[w + 1]]) >= 0) for w in range(n))
    for w in NC.HUBS:                                                   # the transpose is the definition
        assert np.array_equal(t_link[t_ptr[w]:t_ptr[w + 1]],
                              [l for l in range(links.shape[1]) if w in idx[ptr[l]:ptr[l + 1]]])


# ---- refusals that need no device -----------------------------------------------------------------------------------

def test_refusals_without_a_device():
    import scipy.sparse as ssp
    import torch

    from s3grl_amd import ncn

    A = ssp.csr_matrix(np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]]))
    links = np.array([[0], [1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ncn.CommonNeighbours(A, links, device="cpu")
    for flag in (2, -1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="exclude_endpoints"):
            ncn.CommonNeighbours(A, links, exclude_endpoints=flag, device="cpu")
    with pytest.raises(ValueError, match="triple"):
        ncn._graph_on((torch.zeros(4, dtype=torch.int64),), None)
    with pytest.raises(ValueError, match="int64"):
        ncn._graph_on((torch.zeros(4, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), 3), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ncn._graph_on((torch.zeros(4, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 3), None)
    with pytest.raises(ValueError, match="2\\^31"):
        ncn.check_size(1 << 31, 0)
    with pytest.raises(ValueError, match="2\\^31"):
        ncn.check_size(3, 1 << 31)
    with pytest.raises(ValueError):
        ncn._links_on(np.array([[0, 3], [1, 0]]), 3, "cpu")
    with pytest.raises(ValueError):
        ncn._links_on(np.array([[0, -1], [1, 0]]), 3, "cpu")
    with pytest.raises(ValueError):
        ncn._links_on(np.array([[0, 1, 2]]), 3, "cpu")
    lists = ncn.SegmentLists(torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="MI355X only; there is no CPU fallback"):
        ncn.common_neighbour_sum(torch.zeros(3, 4), lists)
    with pytest.raises(TypeError):
        ncn.common_neighbour_sum(torch.zeros(3, 4), object())
    with pytest.raises(RuntimeError, match="MI355X only; there is no CPU fallback"):
        ncn.segment_sum(torch.zeros(3, 4), lists.ptr, lists.idx)
    for bad in (dict(epochs=0), dict(lr=0.0), dict(batch_size=0), dict(hidden=0), dict(dropout=1.0)):
        with pytest.raises(ValueError):
            ncn.run_ncn(None, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ncn.run_ncn(None, device="cpu")
    for bad in (dict(in_channels=0), dict(in_channels=4, hidden=0), dict(in_channels=4, dropout=1.0)):
        with pytest.raises(ValueError):
            ncn.NCNTwin(**bad)
    sig = inspect.signature(ncn.run_ncn).parameters
    assert [sig[k].default for k in ("epochs", "hidden", "lr", "batch_size", "seed", "mask", "use_cn")] == \
        [50, 256, 0.01, 1024, 1, True, True]
    assert inspect.signature(ncn.CommonNeighbours).parameters["exclude_endpoints"].default is True


def test_the_twin_is_the_model_of_the_specification():
    import torch

    from s3grl_amd import ncn

    a, b = ncn.NCNTwin(7, hidden=8, dropout=0.25, seed=3), ncn.NCNTwin(7, hidden=8, dropout=0.25, seed=3)
    assert float(a.beta.detach()) == 1.0 and a.beta.requires_grad and a.encoder.layer == "GCN"
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert a.out.lin2.out_features == 1 and a.xij.lin1.in_features == 8 and a.xcn.lin2.out_features == 8
    assert not torch.equal(a.xij.lin1.weight, ncn.NCNTwin(7, hidden=8, seed=4).xij.lin1.weight)


# ---- the public surface: fails without the feature ----------------------------------------------------------------

def test_the_calls_are_declared_exported_and_refuse_through_the_abi():
    import s3grl_amd
    from s3grl_amd import _native

    import __graft_entry__ as G

    header = (REPO / "include" / "s3grl.h").read_text()
    for name in ("s3grl_cn_count", "s3grl_cn_fill", "s3grl_segment_sum"):
        assert len(re.findall(rf"\b{name}\s*\(", header)) == 1 and name in _native.SYMBOLS
    assert "s3grl_ncn.hip" in G.SOURCES and (REPO / "s3grl_amd" / "csrc" / "s3grl_ncn.hip").exists()
    for name in ("CommonNeighbours", "common_neighbour_sum", "NCNTwin", "run_ncn"):
        assert callable(getattr(s3grl_amd, name))
    from s3grl_amd import ncn

    assert ncn.CHUNK == R.CHUNK == 64
    lib = _native.lib()
    E = _native.ERR_INVALID_ARGUMENT

    def count(n=3, nnz=0, L=0, flag=1):
        return lib.s3grl_cn_count(None, n, None, None, nnz, None, L, flag, None)

    def fill(n=3, nnz=0, L=0, flag=1, total=0):
        return lib.s3grl_cn_fill(None, n, None, None, nnz, None, L, flag, None, total, None)

    def ssum(M=3, H=4, R_=0):
        return lib.s3grl_segment_sum(None, None, M, H, None, None, R_, None)

    assert count() == E and fill() == E and ssum() == E               # null context and arrays
    for bad in (dict(n=0), dict(n=1 << 31), dict(nnz=-1), dict(nnz=1 << 31), dict(L=-1), dict(L=1 << 31),
                dict(flag=2), dict(flag=-1)):
        assert count(**bad) == E and fill(**bad) == E, bad
    assert fill(total=-1) == E
    for bad in (dict(M=-1), dict(M=1 << 31), dict(H=0), dict(H=65537), dict(R_=-1), dict(R_=1 << 31)):
        assert ssum(**bad) == E, bad
    assert "2^31" in lib.s3grl_last_error().decode()
