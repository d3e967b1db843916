"""-m gpu: the packed gather's prefix schedule (pass2 of gather_packed_kernel: a window of W = 64 rows has its
ids and coefficients fetched by vector loads and staged in LDS) on broom graphs whose hop sizes put the prefix
on every edge of that schedule — see prefix_graphs.py for the table and test_gather_prefix_host.py for the
proof that the table produces those lengths.

The expected rows are restated on the host without any code of the kernel: per output column the addends in
LIST order (hop-major; inside a hop by the graph's degree order, the two endpoints first) through
single-rounded fp32 multiply-adds (prefix_fma.fma32); a list gathered in pieces as the pieces' chains, added
in fp64 in ascending order.  The coefficients are the plan's own: the same plan run
on the identity matrix through the DENSE gather hands back, per row and operator, the coefficient of every
node (c * 1 + 0 is exact).  `auto` (element rows: one launch or two), `packed_only` (chunk path) must equal
it bit for bit, the dense operand within 1e-6, and the fp64 C restatement is met at the parity bar.

Mutations of the kernel that this file caught when it was written (each built once, run once, not kept):
the last row of a window dropped; an operator's coefficient run read one row late."""
import numpy as np
import pytest

import prefix_graphs as pg
from conftest import csr_from_undirected
from oracle import c_oracle
from prefix_fma import fma32

pytestmark = pytest.mark.gpu

F = 530             # two tiles of 512 columns, the last ragged
HOPS = 3
TOL, ATOL = 1e-5, 1e-10   # the parity bar of test_gpu_parity.py


@pytest.fixture(scope="module")
def eng():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    e = Engine("cuda:0")
    yield e
    e.close()


def _operand(n, density, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, F)) * (rng.random((n, F)) < density)).astype(np.float32)


class Scene:
    """The brooms with or without reversed duplicates, their CSR, the list order of every link and the operands."""

    def __init__(self, rev):
        self.n, self.edges, self.links = pg.brooms(reversed_links=rev)
        self.A = csr_from_undirected(self.n, self.edges)
        deg = np.diff(self.A.indptr)
        rank = np.empty(self.n, dtype=np.int64)     # the graph's degree order: degree descending, id ascending
        rank[np.lexsort((np.arange(self.n), -deg))] = np.arange(self.n)
        self.order, self.sizes = [], []
        for l in self.links:
            hops = pg.hop_lists(self.n, self.edges, l)[:HOPS + 1]
            self.order.append(np.concatenate([h[np.argsort(rank[h], kind="stable")] for h in hops]))
            self.sizes.append([len(h) for h in hops])
        # 15 % of the entries: ~40 per row-tile, the two-launch element plan; 4 %: ~10, the one-launch kernel
        self.X = {"x15": _operand(self.n, 0.15, 3), "x4": _operand(self.n, 0.04, 4)}
        assert (self.X["x15"] < 0).any() and (self.X["x15"] != 0).sum() >= 24 * 2 * self.n
        assert (self.X["x4"] != 0).sum() < 24 * 2 * self.n
        self._coef, self._exp, self._ref = {}, {}, {}


@pytest.fixture(scope="module")
def scenes():
    return {rev: Scene(rev) for rev in (False, True)}


def _coefficients(eng, S, G, mode, K):
    """(rows [R, K+1, 1+n] of the plan on the identity through the dense gather, row_ptr, row_nodes)"""
    key = (mode, K)
    if key not in S._coef:
        f = eng.features(np.eye(S.n, dtype=np.float32), "dense")
        assert not f.is_packed and not f.is_sparse
        res = eng.precompute(G, f, eng.links(S.links.T.copy()), mode=mode, num_hops=HOPS, sign_k=K)
        f.close()
        S._coef[key] = (res.rows.cpu().numpy(), res.row_ptr.cpu().numpy(), res.row_nodes.cpu().numpy())
    return S._coef[key]


SPLIT_T = 48        # the hooks of the `pieces` cases (as test_gpu_element_split.py sets them)


def _chain(c, X, order):
    """[rows, K, F]: per column the fp32 multiply-add chain over `order`, from zero"""
    acc = np.zeros(c.shape[:2] + (F,), dtype=np.float32)
    for j, v in enumerate(order):
        acc = fma32(c[:, :, j, None], X[v][None, None, :], acc)
    return acc


def _expected(eng, S, G, mode, K, xname, split):
    """A list longer than SPLIT_T rows is gathered in pieces of pg.SEG rows when `split`: every piece its own
    chain from zero, the pieces' fp32 rows added in ascending order in fp64 and rounded once (combine_kernel).
    The list of a row pair ends with the last hop its last operator reaches: hop K for the endpoints' pair,
    hop K + 1 for a pair of common neighbours (which sit at hop 1), at most HOPS."""
    key = (mode, K, xname, split)
    if key not in S._exp:
        crow, ptr, nodes = _coefficients(eng, S, G, mode, K)
        X = S.X[xname]
        exp = np.zeros((crow.shape[0], K + 1, F + 1), dtype=np.float32)
        exp[:, :, 0] = crow[:, :, 0]          # the label column does not depend on the operand
        exp[:, 0, 1:] = X[nodes]
        for li, (order, sizes) in enumerate(zip(S.order, S.sizes)):
            for r0 in range(ptr[li], ptr[li + 1], 2):        # row pairs: the endpoints, then the common neighbours
                r1 = min(r0 + 2, ptr[li + 1])
                support = int(sum(sizes[:min(K + (1 if r0 > ptr[li] else 0), HOPS) + 1]))
                lst = order[:support]
                c = crow[r0:r1, 1:, :][:, :, 1 + lst]            # [rows, K, list]
                assert not crow[r0:r1, 1:, 1:][:, :, np.setdiff1d(np.arange(S.n), lst)].any()
                if split and support > SPLIT_T:
                    acc = np.zeros((r1 - r0, K, F), dtype=np.float64)
                    for s0 in range(0, support, pg.SEG):
                        acc += _chain(c[:, :, s0:s0 + pg.SEG], X, lst[s0:s0 + pg.SEG]).astype(np.float64)
                    acc = acc.astype(np.float32)
                else:
                    acc = _chain(c, X, lst)
                exp[r0:r1, 1:, 1:] = acc
        S._exp[key] = (exp, ptr, nodes)
    return S._exp[key]


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=-1, keepdims=True))
    return float(np.max(np.clip(np.abs(got - ref) - ATOL, 0, None) / np.maximum(scale, 1e-30)))


def _oracle(S, mode, K, xname):
    key = (mode, K, xname)
    if key not in S._ref:
        S._ref[key] = c_oracle.pos_rows(S.links.T, HOPS, S.A, S.X[xname], K, plus=mode == "pos_plus")[:3]
    return S._ref[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("xname", ["x15", "x4"])
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("split", [False, True], ids=["whole", "pieces"])
@pytest.mark.parametrize("rev", [False, True], ids=["plain", "reversed"])
@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
def test_prefix_schedule_bits(eng, scenes, monkeypatch, mode, rev, split, K, xname):
    S = scenes[rev]
    G = eng.graph(S.A)
    exp, ptr, nodes = _expected(eng, S, G, mode, K, xname, split)   # (its plan on the identity: before the hooks below)
    ref, ref_ptr, ref_nodes = _oracle(S, mode, K, xname)
    np.testing.assert_array_equal(ptr, ref_ptr)
    np.testing.assert_array_equal(nodes, ref_nodes)
    if mode == "pos_plus":
        assert (np.diff(ptr) == 3).all()      # every broom has its one common neighbour: a pair with row_hop = 1
    if split:
        monkeypatch.setenv("S3GRL_SPLIT_T", str(SPLIT_T))
        monkeypatch.setenv("S3GRL_SPLIT_SEG_SHIFT", "4")
    links = eng.links(S.links.T.copy())
    plan = eng.plan(G, links, mode=mode, num_hops=HOPS, sign_k=K)
    try:
        np.testing.assert_array_equal(plan.row_ptr().cpu().numpy(), ptr)
        if rev:
            assert plan.folded_links == len(S.links) // 2
        if split:
            assert plan.stats["max_nodes"] > SPLIT_T
        for fmode in ("auto", "packed_only", "dense"):
            f = eng.features(S.X[xname], fmode)
            got = plan.run(f).cpu().numpy()
            if fmode != "dense":
                assert f.is_packed
                t = plan.gather_traffic(f)
                # which kernels ran: only the two-launch element plan fetches 8 header bytes (the element
                # range) instead of 32 for the rows of its phase-B launch
                two_launches = fmode == "auto" and xname == "x15" and K - 1 < HOPS
                assert (t["headers"] < 8 * t["ids"]) == two_launches, (fmode, t)
                if fmode == "auto" and K - 1 < HOPS:
                    assert t["features"] < plan_chunk_bytes(plan, eng, S, xname)   # element rows were read
            f.close()
            if fmode == "dense":
                assert rel_err(got, exp) < 1e-6
            else:
                bad = np.argwhere(_bits(got) != _bits(exp))
                assert not len(bad), (fmode, len(bad), bad[:4].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
            err = rel_err(got, ref)
            assert err < TOL, (fmode, err)
    finally:
        plan.close()
        G.close()


def plan_chunk_bytes(plan, eng, S, xname):
    f = eng.features(S.X[xname], "packed_only")
    try:
        return plan.gather_traffic(f)["features"]
    finally:
        f.close()
