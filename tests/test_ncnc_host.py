"""CPU checks of the NCNC restatement (tests/ncnc_reference.py): the three sections against dense
boolean masks and against a rebuild without the link's own entries; S0 against the NCN restatement; the weighted sum
with unit weights against the unweighted one, to the byte; sum, dot and z-gradient against fp64 within the derived
bound; the four named faults against byte equality, each on a case built for it; the twin's state_dict; the refusals
that need no device; and the public surface of the four new symbols."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as ssp

import ncn_cases as NC
import ncn_reference as NR
import ncnc_reference as R

REPO = Path(__file__).resolve().parent.parent


def _differ(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return int(np.count_nonzero(a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)))


def _sections(counts, ptr, idx, side, l):
    """the three sections of link l, with the layout checked: side is 0.., 1.., 2.. in the lengths counts gives"""
    n0, n1, n2 = counts[:, l].tolist()
    b = int(ptr[l])
    assert ptr[l + 1] - b == n0 + n1 + n2
    assert side[b:b + n0 + n1 + n2].tolist() == [0] * n0 + [1] * n1 + [2] * n2
    return idx[b:b + n0], idx[b + n0:b + n0 + n1], idx[b + n0 + n1:b + n0 + n1 + n2]


# ---- the sections ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", (False, True))
@pytest.mark.parametrize("name", ("random", "directed", "hub", "lengths"))
def test_sections_equal_dense_masks(name, flag):
    A, links = NC.list_cases()[name]
    D = np.asarray(ssp.csr_matrix(A).todense()) != 0
    counts, ptr, idx, side = R.split_lists(A, links, flag)
    assert counts.dtype == np.int64 and counts.shape == (3, links.shape[1]) and ptr.dtype == np.int64
    assert idx.dtype == np.int32 and side.dtype == np.int32 and len(idx) == len(side) == ptr[-1]
    loops = D.diagonal()
    u, v = links
    if name == "lengths":                                   # u == v, and a self-loop at either endpoint
        assert (u == v).any() and (loops[u] & ~loops[v]).any() and (~loops[u] & loops[v]).any()
    for l, (a, b) in enumerate(links.T.tolist()):
        masks = [D[a] & D[b], D[a] & ~D[b], ~D[a] & D[b]]
        for got, m in zip(_sections(counts, ptr, idx, side, l), masks):
            if flag:
                m = m.copy()
                m[[a, b]] = False
            assert np.array_equal(got, np.nonzero(m)[0]), (name, flag, a, b)
        if a == b:
            assert counts[1, l] == 0 and counts[2, l] == 0
    cn_ptr, cn_idx = NR.cn_lists(A, links, flag)            # S0 is the NCN list
    s0 = [_sections(counts, ptr, idx, side, l)[0] for l in range(links.shape[1])]
    assert np.array_equal(np.diff(cn_ptr), counts[0])
    assert np.array_equal(np.concatenate(s0) if len(s0) else np.zeros(0, np.int32), cn_idx)


@pytest.mark.parametrize("name", ("random", "hub"))
def test_the_flag_equals_a_rebuild_without_the_links_own_entries_where_there_are_no_self_loops(name):
    A, links = NC.list_cases()[name]
    A = ssp.lil_matrix(A)
    A.setdiag(0)                                            # the hub graph has five self-loops: they leave
    A = ssp.csr_matrix(A)
    A.eliminate_zeros()
    assert A.diagonal().sum() == 0
    links = links[:, :60]
    counts, ptr, idx, side = R.split_lists(A, links, True)
    changed = 0
    for l, (a, b) in enumerate(links.T.tolist()):
        c2, p2, i2, s2 = R.split_lists(NC.without_link(A, a, b), np.array([[a], [b]]), False)
        for got, ref in zip(_sections(counts, ptr, idx, side, l), _sections(c2, p2, i2, s2, 0)):
            assert np.array_equal(got, ref), (a, b)
        c0 = R.split_lists(A, np.array([[a], [b]]), False)[0]
        changed += int(c0.sum() != c2.sum())
    assert changed                                          # some link's own entry was stored: the flag did something


def test_inner_pairs_are_the_missing_edges_in_entry_order():
    A, links = NC.list_cases()["directed"]
    D = np.asarray(ssp.csr_matrix(A).todense()) != 0
    counts, ptr, idx, side = R.split_lists(A, links, True)
    at, pairs = R.inner_pairs(links, ptr, idx, side)
    assert pairs.dtype == np.int32 and pairs.shape == (2, len(at)) and np.array_equal(at, np.nonzero(side)[0])
    owner = np.repeat(np.arange(links.shape[1]), np.diff(ptr))[at]
    for j, l, (a, b) in zip(at.tolist(), owner.tolist(), pairs.T.tolist()):
        u, v = links[:, l]
        if side[j] == 1:
            assert (a, b) == (idx[j], v) and D[u, a] and not D[v, a]
        else:
            assert (a, b) == (u, idx[j]) and D[v, b] and not D[u, b]


# ---- the weighted sum, the dot and the gradient in z ----------------------------------------------------------------

def test_unit_weights_give_the_unweighted_sum_to_the_byte():
    M, ptr, idx = NC.segment_case()
    h = R.values((M, 5), seed=5)
    h[7, 0] = -0.0
    got = R.segment_wsum(h, ptr, idx, np.ones(len(idx), np.float32))
    assert _differ(got, NR.segment_sum(h, ptr, idx)) == 0
    assert np.signbit(got[-1, 0])                           # 300 repeats of -0.0 stay -0.0 under weight 1.0


def test_sum_dot_and_gradient_lie_within_the_derived_bound_of_fp64():
    """A term is one rounded product and a sum of n terms adds n - 1 roundings on its longest path: n roundings,
    n·2^-24·Σ|terms| to first order, whatever the order of the additions."""
    A, links = NC.autograd_case()
    n, L = A.shape[0], links.shape[1]
    _, ptr, idx, _ = R.split_lists(A, links, True)
    H = 5
    z, g, w = R.values((n, H), seed=1), R.values((L, H), seed=2), R.weights(len(idx), seed=3)
    owner = np.repeat(np.arange(L), np.diff(ptr))
    W = np.zeros((L, n))
    W[owner, idx] = w.astype(np.float64)
    held = np.zeros((L, n))
    held[owner, idx] = 1.0
    z64, g64 = z.astype(np.float64), g.astype(np.float64)
    eps = 2.0 ** -24
    fwd = R.segment_wsum(z, ptr, idx, w).astype(np.float64)
    assert np.all(np.abs(fwd - W @ z64) <= held.sum(1, keepdims=True) * eps * (np.abs(W) @ np.abs(z64)))
    grad = R.wsum_grad_z(g, ptr, idx, w, n).astype(np.float64)
    assert np.all(np.abs(grad - W.T @ g64) <= held.sum(0)[:, None] * eps * (np.abs(W).T @ np.abs(g64)))
    assert held.sum(0).max() > 2 * R.CHUNK and held.sum(1).max() > R.CHUNK
    for Hd in (5, 130, 260):
        zz, gg = R.values((n, Hd), seed=4), R.values((L, Hd), seed=5)
        dot = R.segment_dot(gg, zz, ptr, idx).astype(np.float64)
        terms = gg.astype(np.float64)[owner] * zz.astype(np.float64)[idx]
        assert np.all(np.abs(dot - terms.sum(1)) <= Hd * eps * np.abs(terms).sum(1))


# ---- the named faults leave byte equality --------------------------------------------------------------------------

def test_fault_contracted_moves_an_ulp_on_a_row_of_mixed_exponents():
    h = R.values((40, 16), seed=7)
    idx = np.random.default_rng(7).integers(0, 40, 9).astype(np.int32)
    ptr, w = np.array([0, 2, 9], np.int64), R.values((9,), seed=8)
    good, bad = R.segment_wsum(h, ptr, idx, w), R.segment_wsum(h, ptr, idx, w, fault="contracted")
    print(f"[ncnc] contracted: {_differ(good, bad)} bytes differ; the row of 2 entries: {_differ(good[:1], bad[:1])}")
    assert _differ(good[:1], bad[:1]) > 0 and _differ(good[1:], bad[1:]) > 0
    assert np.allclose(good, bad, rtol=0, atol=1e-5)
    one = np.array([0, 1], np.int64)                        # a single term: nothing to contract with
    assert _differ(R.segment_wsum(h, one, idx[:1], w[:1]), R.segment_wsum(h, one, idx[:1], w[:1], fault="contracted")) == 0


def test_fault_sequential_dot_moves_an_ulp_at_130_columns():
    g, h = R.values((3, 130), seed=9), R.values((50, 130), seed=10)
    ptr, idx = np.array([0, 4, 4, 12], np.int64), np.random.default_rng(9).integers(0, 50, 12).astype(np.int32)
    good, bad = R.segment_dot(g, h, ptr, idx), R.segment_dot(g, h, ptr, idx, fault="sequential_dot")
    print(f"[ncnc] sequential_dot: {_differ(good, bad)} bytes differ over 12 dots of 130 columns")
    assert _differ(good, bad) > 0 and np.allclose(good, bad, rtol=0, atol=1e-4)
    # four columns are one slot: the two orders are the same order
    assert _differ(R.segment_dot(g[:, :4], h[:, :4], ptr, idx),
                   R.segment_dot(g[:, :4], h[:, :4], ptr, idx, fault="sequential_dot")) == 0


def test_fault_s2_before_s1_moves_the_entries():
    A, links = NC.length_graph()
    counts, ptr, idx, side = R.split_lists(A, links, True)
    c2, p2, i2, s2 = R.split_lists(A, links, True, fault="s2_before_s1")
    assert ((counts[1] > 0) & (counts[2] > 0)).any()
    assert np.array_equal(counts, c2) and np.array_equal(ptr, p2)
    assert _differ(idx, i2) > 0 and _differ(side, s2) > 0


def test_fault_forward_weights_moves_the_gradient():
    A, links = NC.autograd_case()
    n = A.shape[0]
    _, ptr, idx, _ = R.split_lists(A, links, True)
    g, w = R.values((links.shape[1], 8), seed=11), R.weights(len(idx), seed=12)
    good, bad = R.wsum_grad_z(g, ptr, idx, w, n), R.wsum_grad_z(g, ptr, idx, w, n, fault="forward_weights")
    assert _differ(good, bad) > 0
    order = np.argsort(idx, kind="stable")
    assert np.array_equal(R.transposed_weights(w, ptr, idx), w[order]) and not np.array_equal(order, np.arange(len(idx)))
    ones = np.ones(len(idx), np.float32)                    # with equal weights the order of the weights is moot
    assert _differ(R.wsum_grad_z(g, ptr, idx, ones, n), R.wsum_grad_z(g, ptr, idx, ones, n, fault="forward_weights")) == 0
    assert _differ(R.wsum_grad_z(g, ptr, idx, ones, n), NR.cn_sum_grad(g, ptr, idx, n)) == 0


# ---- the twin and the refusals that need no device ------------------------------------------------------------------

def test_the_ncnc_twin_loads_an_ncn_state_dict():
    import torch

    from s3grl_amd import ncn

    a, b = ncn.NCNTwin(7, hidden=8, dropout=0.25, seed=3), ncn.NCNCTwin(7, hidden=8, dropout=0.25, seed=5)
    assert list(a.state_dict()) == list(b.state_dict())
    assert {k.split(".")[0] for k in b.state_dict()} == {"encoder", "xij", "xcn", "out", "beta"}
    assert not torch.equal(a.xcn.lin1.weight, b.xcn.lin1.weight)
    b.load_state_dict(a.state_dict())
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))
    assert b.detach_completion is False and ncn.NCNCTwin(7, hidden=8, detach_completion=True).detach_completion is True
    assert isinstance(b, ncn.NCNTwin)


def test_refusals_without_a_device():
    import torch

    from s3grl_amd import ncn

    A = ssp.csr_matrix(np.array([[0, 1, 1], [1, 0, 1], [1, 1, 0]]))
    links = np.array([[0], [1]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ncn.SplitNeighbours(A, links, device="cpu")
    for flag in (2, -1, "yes", None, 1.0):
        with pytest.raises(ValueError, match="exclude_endpoints"):
            ncn.SplitNeighbours(A, links, exclude_endpoints=flag, device="cpu")
    lists = ncn.SegmentLists(torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="MI355X only; there is no CPU fallback"):
        ncn.completed_neighbour_sum(torch.zeros(3, 4), lists, torch.zeros(0))
    with pytest.raises(TypeError):
        ncn.completed_neighbour_sum(torch.zeros(3, 4), object(), torch.zeros(0))
    with pytest.raises(TypeError):
        ncn.completed_neighbour_sum(torch.zeros(3, 4), lists, None)
    for bad in (dict(epochs=0), dict(lr=0.0), dict(batch_size=0), dict(hidden=0), dict(dropout=1.0)):
        with pytest.raises(ValueError):
            ncn.run_ncnc(None, **bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ncn.run_ncnc(None, device="cpu")
    for bad in (dict(in_channels=0), dict(in_channels=4, hidden=0), dict(in_channels=4, dropout=1.0)):
        with pytest.raises(ValueError):
            ncn.NCNCTwin(**bad)
    sig, ref = inspect.signature(ncn.run_ncnc).parameters, inspect.signature(ncn.run_ncn).parameters
    assert list(sig) == [k for k in ref if k != "use_cn"]
    assert all(sig[k].default == ref[k].default for k in sig)
    assert inspect.signature(ncn.SplitNeighbours).parameters["exclude_endpoints"].default is True
    assert inspect.signature(ncn.NCNCTwin).parameters["detach_completion"].default is False


# ---- the public surface: fails without the feature ----------------------------------------------------------------

def test_the_calls_are_declared_exported_and_refuse_through_the_abi():
    import s3grl_amd
    from s3grl_amd import _native

    header = (REPO / "include" / "s3grl.h").read_text()
    for name in ("s3grl_cn_split_count", "s3grl_cn_split_fill", "s3grl_segment_wsum", "s3grl_segment_dot"):
        assert len(re.findall(rf"\b{name}\s*\(", header)) == 1, name
        assert _native.SYMBOLS.count(name) == 1, name
    for name in ("SplitNeighbours", "completed_neighbour_sum", "NCNCTwin", "run_ncnc"):
        assert callable(getattr(s3grl_amd, name))
    lib = _native.lib()
    E = _native.ERR_INVALID_ARGUMENT

    def count(n=3, nnz=0, L=0, flag=1):
        return lib.s3grl_cn_split_count(None, n, None, None, nnz, None, L, flag, None)

    def fill(n=3, nnz=0, L=0, flag=1, total=0):
        return lib.s3grl_cn_split_fill(None, n, None, None, nnz, None, L, flag, None, None, total, None, None)

    def wsum(M=3, H=4, R_=0):
        return lib.s3grl_segment_wsum(None, None, M, H, None, None, None, R_, None)

    def dot(M=3, H=4, R_=0):
        return lib.s3grl_segment_dot(None, None, R_, None, M, H, None, None, None)

    assert count() == E and fill() == E and wsum() == E and dot() == E        # null context and arrays
    for bad in (dict(n=0), dict(n=1 << 31), dict(nnz=-1), dict(L=-1), dict(flag=2)):
        assert count(**bad) == E and fill(**bad) == E, bad
    assert fill(total=-1) == E
    for bad in (dict(H=0), dict(H=65537), dict(R_=-1), dict(M=1 << 31), dict(R_=1 << 31)):
        assert wsum(**bad) == E and dot(**bad) == E, bad
    assert "2^31" in lib.s3grl_last_error().decode()
