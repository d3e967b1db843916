"""The masked pairs kernel (csrc/s3grl_sketch.hip: sketch_masked_pairs_kernel behind s3grl_masked_sketch_pairs, and
`SketchGraph.features / intersections / raw(links, mask=True)`) against the numpy restatement
(tests/sketch_mask_reference.py; tests/test_sketch_mask_host.py shows that it equals one rebuild of the sketches per
link and that its named faults leave the comparison used here) and against the merged unmasked path on the graph
without the link (`SketchGraph(A⁻)`), an oracle that shares no code with the masked kernel's walk.

Every comparison is equality of bytes and prints how many entries are unequal.  Calls through the C ABI fill their
outputs with sentinels first (-1, NaN), so an entry the kernel fails to write cannot pass."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import sketch_mask_cases as MC
import sketch_mask_reference as MR
import sketch_reference as R

pytestmark = pytest.mark.gpu

HOPS = (1, 2)
SHAPES = ((64, 7), (128, 8), (192, 9), (512, 10))      # 1, 1, 2 and 4 columns per lane


def _engine():
    from s3grl_amd.engine import default_engine

    return default_engine()


def _np(t):
    return t.detach().cpu().numpy()


def _same(what, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    differ = int(np.count_nonzero(got.view(np.uint8).reshape(-1) != ref.view(np.uint8).reshape(-1))) if got.size else 0
    entries = int(np.count_nonzero(got != ref)) if got.size else 0
    print(f"[mask] {what}: {entries} of {got.size} entries unequal ({differ} bytes)")
    assert differ == 0, what


class _Tables:
    """The CSR and the unmasked tables of a graph on the device, built through the C ABI."""

    def __init__(self, A, hops, P, p, seed=0):
        from s3grl_amd import _native as N
        from s3grl_amd import sketch as S
        from s3grl_amd.heuristics import canonical_csr

        A = canonical_csr(A)
        eng = _engine()
        self.n, self.nnz, self.hops, self.P, self.p = A.shape[0], int(A.nnz), hops, P, p
        self.ip = torch.as_tensor(A.indptr.astype(np.int64)).to(eng.device)
        self.ix = torch.as_tensor(A.indices.astype(np.int32)).to(eng.device)
        self.mh = torch.full((hops + 1, self.n, P), -1, dtype=torch.int32, device=eng.device)
        self.hl = torch.full((hops + 1, self.n, 1 << p), 0xFF, dtype=torch.uint8, device=eng.device)
        N.check(N.lib().s3grl_sketch_build(eng._ctx, self.n, N.ptr(self.ip), N.ptr(self.ix), self.nnz, hops, P, p, seed,
                                           N.ptr(self.mh), N.ptr(self.hl)), "s3grl_sketch_build")
        _, self.C, lc = S.hll_constants(p)
        self.lc = torch.as_tensor(lc).to(eng.device)
        torch.cuda.synchronize()

    def pairs(self, links, mask, want=MR.NAMES):
        """s3grl_masked_sketch_pairs (or s3grl_sketch_pairs) into sentinel-filled outputs -> {name: numpy}"""
        from s3grl_amd import _native as N

        eng, K1, L = _engine(), self.hops + 1, links.shape[1]
        l_d = torch.as_tensor(np.ascontiguousarray(links, dtype=np.int32)).to(eng.device)
        out = {"match": torch.full((L, K1, K1), -1, dtype=torch.int32, device=eng.device),
               "T": torch.full((L, K1, K1), -1, dtype=torch.int64, device=eng.device),
               "z": torch.full((L, K1, K1), -1, dtype=torch.int32, device=eng.device),
               "intersections": torch.full((L, K1, K1), float("nan"), dtype=torch.float32, device=eng.device),
               "features": torch.full((L, self.hops * self.hops + 2 * self.hops), float("nan"), dtype=torch.float32,
                                      device=eng.device)}
        outs = [N.ptr(out[k]) if k in want else None for k in out]
        if mask:
            N.check(N.lib().s3grl_masked_sketch_pairs(eng._ctx, self.n, N.ptr(self.ip), N.ptr(self.ix), self.nnz,
                                                      self.hops, self.P, self.p, N.ptr(self.mh), N.ptr(self.hl),
                                                      N.ptr(self.lc), self.C, N.ptr(l_d), L, *outs),
                    "s3grl_masked_sketch_pairs")
        else:
            N.check(N.lib().s3grl_sketch_pairs(eng._ctx, self.n, self.hops, self.P, self.p, N.ptr(self.mh),
                                               N.ptr(self.hl), N.ptr(self.lc), self.C, N.ptr(l_d), L, *outs),
                    "s3grl_sketch_pairs")
        torch.cuda.synchronize()
        return {k: _np(v) for k, v in out.items()}


@lru_cache(maxsize=None)
def _reference(name, hops, P, p, seed):
    """(unmasked tables, masked restatement of the case's links and of the reversed links), computed once"""
    A, links = MC.every_case()[name]
    mh, hl = R.sketches(A, hops, P, p, seed)
    return mh, hl, MR.masked_link_outputs(A, mh, hl, links, p), MR.masked_link_outputs(A, mh, hl, links[::-1], p)


def _check_case(name, hops, P, p, seed=0):
    A, links = MC.every_case()[name]
    _, _, ref_uv, ref_vu = _reference(name, hops, P, p, seed)
    tab = _Tables(A, hops, P, p, seed)
    got = {}
    for order, ll, ref in (("(u, v)", links, ref_uv), ("(v, u)", links[::-1].copy(), ref_vu)):
        got[order] = tab.pairs(ll, mask=True)
        for k in MR.NAMES:
            _same(f"{name} hops {hops} P {P} p {p} {order} {k}", got[order][k], ref[k])
        assert not np.isnan(got[order]["features"]).any() and not np.isnan(got[order]["intersections"]).any()
    for k in ("match", "T", "z", "intersections"):
        assert np.array_equal(got["(v, u)"][k].view(np.uint8),
                              np.ascontiguousarray(got["(u, v)"][k].transpose(0, 2, 1)).view(np.uint8)), k
    return tab, got["(u, v)"]


# ---- byte equality at every lane layout, on every kind of link ---------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"P{s[0]}p{s[1]}")
@pytest.mark.parametrize("hops", HOPS)
def test_masked_outputs_equal_the_restatement(hops, shape):
    """Every case of sketch_mask_cases: links stored both ways, one way in either orientation and not at all, u == v
    with and without a self-loop, an endpoint with a self-loop, a degree-1 endpoint whose only key is the partner,
    an isolated node, masked rows of 0 .. 65 keys, and the long rows."""
    P, p = shape
    for name in MC.every_case():
        _check_case(name, hops, P, p, seed=hops * 1000 + P)


@pytest.mark.parametrize("hops", HOPS)
def test_row_lengths_of_the_masked_endpoint(hops):
    """0, 1, 2, 3, 4, 5 (the batch and its remainder), 63, 64 and 65 keys (65: past kSplitKeys, a quarter of 17 keys
    per wavefront), at the defaults; every masked link's features differ from the unmasked ones or its masked rows
    equal the table rows."""
    A, links = MC.length_case()
    deg = np.diff(A.indptr)
    st = MC.stored(A, links)
    assert sorted(set(deg[links[0]][st[0]].tolist())) == [d for d in MC.LENGTHS if d]
    tab, got = _check_case("lengths", hops, 128, 8)
    plain = tab.pairs(links, mask=False)
    changed = (got["features"].view(np.uint32) != plain["features"].view(np.uint32)).any(axis=1)
    print(f"[mask] lengths hops {hops}: {int(changed[st.any(axis=0)].sum())} of {int(st.any(axis=0).sum())} change")
    assert 2 * int(changed.sum()) >= int(st.any(axis=0).sum())


@pytest.mark.parametrize("hops", HOPS)
def test_split_rows_at_every_partner_position(hops):
    """Rows of 600 / 601 and 260 / 261 keys walked by the workgroup's four wavefronts: the partner first, last, inside
    every quarter and on both sides of every quarter boundary; both endpoints long (0, 1), only one long with the
    other masked too (the short rows that point back), only one long with the other not stored (the directed hub)."""
    for name in ("hub", "long"):
        A, links = MC.every_case()[name]
        deg, st = np.diff(A.indptr), MC.stored(A, links)
        long_u = deg[links[0]] > MC.SPLIT_KEYS
        row0 = A.indices[A.indptr[0]:A.indptr[1]]
        at = {int(np.searchsorted(row0, v)) for u, v in links.T[st[0] & long_u] if u == 0}
        assert set(MC.quarter_positions(len(row0))) <= at, (name, sorted(at))
        _check_case(name, hops, 128, 8)
    A, links = MC.long_case()
    deg, st = np.diff(A.indptr), MC.stored(A, links)
    both = st[0] & st[1]
    assert (both & (deg[links[0]] > 64) & (deg[links[1]] > 64)).any()
    assert (both & (deg[links[0]] > 64) & (deg[links[1]] <= 64)).any()


# ---- link lists ---------------------------------------------------------------------------------------------------

def test_link_list_sizes_repeats_and_outputs_asked_for():
    """0, 1, 2, 3, 5 and 11 links: workgroups with dead wavefronts beside a long-row link, which still meet every
    barrier.  A repeated link gives equal rows, its reverse the transposes; only the outputs asked for are written."""
    A, _ = MC.long_case()
    row0 = A.indices[A.indptr[0]:A.indptr[1]]
    w = int(row0[300])
    base = np.array([[0, 0, 7, w, 0, 1, 2, 3, 0, 899, 5], [1, w, 7, 0, w, 0, 2, 3, 1, 899, 6]], dtype=np.int64)
    mh, hl = R.sketches(A, 2, 128, 8, 0)
    tab = _Tables(A, 2, 128, 8)
    for L in (0, 1, 2, 3, 5, 11):
        links = base[:, :L]
        ref, got = MR.masked_link_outputs(A, mh, hl, links, 8), tab.pairs(links, mask=True)
        for k in MR.NAMES:
            _same(f"L = {L} {k}", got[k], ref[k])
    got = tab.pairs(base, mask=True)
    for k in MR.NAMES:
        assert np.array_equal(got[k][1].view(np.uint8), got[k][4].view(np.uint8)), k                 # a repeat
        assert np.array_equal(got[k][0].view(np.uint8), got[k][8].view(np.uint8)), k
    for k in ("match", "T", "z", "intersections"):
        assert np.array_equal(got[k][3].view(np.uint8), np.ascontiguousarray(got[k][1].T).view(np.uint8)), k
        assert np.array_equal(got[k][5].view(np.uint8), np.ascontiguousarray(got[k][0].T).view(np.uint8)), k
    some = tab.pairs(base, mask=True, want=("features",))
    assert np.all(some["match"] == -1) and np.all(some["T"] == -1) and np.isnan(some["intersections"]).all()
    assert np.array_equal(some["features"].view(np.uint8), got["features"].view(np.uint8))
    ints = tab.pairs(base, mask=True, want=("match", "T", "z"))
    assert np.isnan(ints["features"]).all() and np.array_equal(ints["T"], got["T"])
    from s3grl_amd import sketch as S

    sk = S.SketchGraph(A)
    try:
        assert tuple(sk.features(np.zeros((2, 0), dtype=np.int64), mask=True).shape) == (0, 8)
        assert tuple(sk.intersections(torch.zeros((2, 0), dtype=torch.long), mask=True).shape) == (0, 3, 3)
        assert [tuple(t.shape) for t in sk.raw(np.zeros((2, 0), dtype=np.int64), mask=True)] == [(0, 3, 3)] * 3
    finally:
        sk.close()


# ---- the independent oracle, the default, non-edges, determinism --------------------------------------------------

@pytest.mark.parametrize("hops", HOPS)
def test_masked_equals_the_unmasked_path_on_the_graph_without_the_link(hops):
    """The 32 links of the 300-node graph: masked `raw` and `features` of (u, v) against the merged, unmasked
    `SketchGraph(A⁻).raw / .features`, one build per link, all on the GPU."""
    from s3grl_amd import sketch as S

    A, links = MC.random_case()
    assert links.shape[1] <= 32
    sk = S.SketchGraph(A, hops=hops, seed=3)
    try:
        masked = [_np(t) for t in sk.raw(links, mask=True)] + [_np(sk.features(links, mask=True)),
                                                               _np(sk.intersections(links, mask=True))]
        plain_features = _np(sk.features(links))
    finally:
        sk.close()
    rebuilt = [[] for _ in masked]
    for u, v in links.T:
        one = S.SketchGraph(MR.without_link(A, int(u), int(v)), hops=hops, seed=3)
        try:
            ll = np.array([[u], [v]])
            for at, t in enumerate(list(one.raw(ll)) + [one.features(ll), one.intersections(ll)]):
                rebuilt[at].append(_np(t))
        finally:
            one.close()
    for name, got, ref in zip(("match", "T", "z", "features", "intersections"), masked, rebuilt):
        _same(f"hops {hops} {name} against SketchGraph(A without the link)", got, np.concatenate(ref, axis=0))
    st = MC.stored(A, links).any(axis=0)
    changed = (masked[3].view(np.uint32) != plain_features.view(np.uint32)).any(axis=1)
    print(f"[mask] hops {hops}: {int(changed[st].sum())} of {int(st.sum())} edges change, "
          f"{int(changed[~st].sum())} of {int((~st).sum())} non-edges")
    assert 2 * int(changed[st].sum()) >= int(st.sum()) and not changed[~st].any()


def test_the_default_is_unchanged_non_edges_are_unchanged_and_runs_are_identical():
    from s3grl_amd import sketch as S

    A, links = MC.hub_case()
    mh, hl = R.sketches(A, 2, 128, 8, 5)
    plain_ref = R.link_outputs(mh, hl, links, 8)
    masked_ref = MR.masked_link_outputs(A, mh, hl, links, 8)
    a, b = S.SketchGraph(A, seed=5), S.SketchGraph(A, seed=5)
    try:
        # mask=False and no mask argument: today's path, today's bytes
        for got in (a.features(links), a.features(links, mask=False), a.features(links, False)):
            _same("default features", _np(got), plain_ref["features"])
        _same("default intersections", _np(a.intersections(links, mask=False)), plain_ref["intersections"])
        for k, got in zip(("match", "T", "z"), a.raw(links, mask=False)):
            _same(f"default {k}", _np(got), plain_ref[k])
        # the object's masked calls equal the restatement
        first = {"features": _np(a.features(links, mask=True)), "intersections": _np(a.intersections(links, True))}
        first.update(zip(("match", "T", "z"), (_np(t) for t in a.raw(links, mask=True))))
        for k in MR.NAMES:
            _same(f"object masked {k}", first[k], masked_ref[k])
        # non-edges: the masked outputs are the unmasked ones
        free = ~MC.stored(A, links).any(axis=0)
        assert free.sum() >= 20
        only = links[:, free]
        _same("non-edges features", _np(a.features(only, mask=True)), plain_ref["features"][free])
        for k, got in zip(("match", "T", "z"), a.raw(only, mask=True)):
            _same(f"non-edges {k}", _np(got), plain_ref[k][free])
        # determinism: a second call, another object, a permuted list
        _same("second call", _np(a.features(links, mask=True)), first["features"])
        _same("second object", _np(b.features(links, mask=True)), first["features"])
        perm = np.random.default_rng(3).permutation(links.shape[1])
        _same("permuted list", _np(b.features(links[:, perm], mask=True)), first["features"][perm])
        assert a._indptr.dtype == torch.int64 and a._indices.dtype == torch.int32
        assert a._indptr.numel() == A.shape[0] + 1 and a._indices.numel() == A.nnz
    finally:
        a.close()
        b.close()
    assert a._indptr is None and a._indices is None
    with pytest.raises(RuntimeError, match="closed"):
        a.features(links, mask=True)


def test_bad_input_is_refused_before_any_gpu_work():
    from s3grl_amd import sketch as S

    A, _ = MC.directed_case()
    tab = _Tables(A, 1, 64, 7)
    for bad in ([[0, 40], [1, 0]], [[0, -1], [1, 2]]):
        with pytest.raises(ValueError):
            tab.pairs(np.array(bad), mask=True)
    sk = S.SketchGraph(A, hops=1, num_perm=64, hll_p=7)
    try:
        for bad in ([[0, 40], [1, 0]], [[0, -1], [1, 2]], [[0, 1, 2]]):
            for method in (sk.features, sk.intersections, sk.raw):
                with pytest.raises(ValueError):
                    method(np.array(bad), mask=True)
    finally:
        sk.close()
    deep = S.SketchGraph(A, hops=3)
    try:
        for method in (deep.features, deep.intersections, deep.raw):
            with pytest.raises(NotImplementedError, match="hops <= 2"):
                method(np.array([[0], [1]]), mask=True)
        assert tuple(deep.features(np.array([[0], [1]])).shape) == (1, 15)       # unmasked hops 3 still runs
    finally:
        deep.close()
    tab3 = _Tables(A, 3, 64, 7)
    with pytest.raises(NotImplementedError, match="hops <= 2"):
        tab3.pairs(np.array([[0], [1]]), mask=True)


# ---- end to end ---------------------------------------------------------------------------------------------------

def test_run_buddy_on_usair_masked_beats_unmasked():
    """The packaged USAir topology, seed-0 split, hops 2, 8 epochs, model seed 1, no node features: once unmasked and
    once masked.  Every step's loss is finite and the masked test AUC is strictly above the unmasked one (the numpy
    restatement under a plain torch twin gives 0.938 against 0.849 at these settings with a seed-to-seed spread
    under 0.01).  Both AUCs are printed; no absolute value is asserted."""
    from s3grl_amd import sketch as S
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    split = W.edge_split(n, e, seed=0)
    res, hist = {}, {}
    for mask in (False, True):
        hist[mask] = []
        res[mask] = S.run_buddy(split, hops=2, epochs=8, lr=0.01, seed=1, batch_size=1024, history=hist[mask],
                                mask=mask)
    print(f"[mask] run_buddy USAir, 8 epochs: test AUC unmasked {res[False]['AUC'][1]:.4f}, masked "
          f"{res[True]['AUC'][1]:.4f}; val AUC {res[False]['AUC'][0]:.4f} / {res[True]['AUC'][0]:.4f}")
    assert len(hist[True]) == len(hist[False]) > 0
    assert np.all(np.isfinite(hist[False])) and np.all(np.isfinite(hist[True]))
    assert res[True]["AUC"][1] > res[False]["AUC"][1]
