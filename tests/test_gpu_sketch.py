"""The subgraph-sketch kernels (csrc/s3grl_sketch.hip: sketch_init_kernel, sketch_propagate_kernel,
sketch_cardinality_kernel, sketch_pairs_kernel) against the numpy restatement (tests/sketch_reference.py;
tests/test_sketch_host.py checks it against the definitions and the true sets, and shows that its named faults leave
the comparison used here).

The comparison is equality of bytes, for the integer tables and for the fp32 outputs alike: every integer step is
exact and every fp64 step is one IEEE operation on identical inputs.  Every comparison prints how many
entries are unequal.  Calls through the C ABI fill their outputs with a sentinel first (0xFF bytes, -1, NaN): an entry
the kernels fail to write cannot pass by holding a right answer from an earlier call's memory."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import heuristics_cases as HC
import sketch_cases as K
import sketch_reference as R

pytestmark = pytest.mark.gpu

HOPS = (1, 2, 4)
# (P, p): one MinHash column per lane (half the lanes hold an 8-byte word), two, a ragged third, and eight
SHAPES = ((64, 7), (128, 8), (192, 9), (512, 10))


def _engine():
    from s3grl_amd.engine import default_engine

    return default_engine()


def _np(t):
    return t.detach().cpu().numpy()


def _same(what, got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape, (what, got.dtype, ref.dtype, got.shape, ref.shape)
    differ = int(np.count_nonzero(got.view(np.uint8).reshape(-1) != ref.view(np.uint8).reshape(-1))) if got.size else 0
    entries = int(np.count_nonzero(got != ref)) if got.size else 0
    print(f"[sketch] {what}: {entries} of {got.size} entries unequal to the restatement ({differ} bytes)")
    assert differ == 0, what


def _abi_build(A, hops, P, p, seed=0):
    """s3grl_sketch_build into tables of 0xFF bytes -> (minhash int32, hll uint8) on the device"""
    from s3grl_amd import _native as N
    from s3grl_amd.heuristics import canonical_csr

    A = canonical_csr(A)
    eng, n = _engine(), A.shape[0]
    ip = torch.as_tensor(A.indptr.astype(np.int64)).to(eng.device)
    ix = torch.as_tensor(A.indices.astype(np.int32)).to(eng.device)
    mh = torch.full((hops + 1, n, P), -1, dtype=torch.int32, device=eng.device)
    hl = torch.full((hops + 1, n, 1 << p), 0xFF, dtype=torch.uint8, device=eng.device)
    N.check(N.lib().s3grl_sketch_build(eng._ctx, n, N.ptr(ip), N.ptr(ix), int(A.nnz), hops, P, p, seed, N.ptr(mh),
                                       N.ptr(hl)), "s3grl_sketch_build")
    torch.cuda.synchronize()
    return mh, hl


def _abi_pairs(mh, hl, p, links, want=("match", "T", "z", "intersections", "features")):
    """s3grl_sketch_pairs into sentinel-filled outputs -> {name: numpy}"""
    from s3grl_amd import _native as N
    from s3grl_amd import sketch as S

    eng = _engine()
    K1, n, P = mh.shape
    hops, L = K1 - 1, links.shape[1]
    _, C, lc = S.hll_constants(p)
    lc = torch.as_tensor(lc).to(eng.device)
    l_d = torch.as_tensor(np.ascontiguousarray(links, dtype=np.int32)).to(eng.device)
    out = {"match": torch.full((L, K1, K1), -1, dtype=torch.int32, device=eng.device),
           "T": torch.full((L, K1, K1), -1, dtype=torch.int64, device=eng.device),
           "z": torch.full((L, K1, K1), -1, dtype=torch.int32, device=eng.device),
           "intersections": torch.full((L, K1, K1), float("nan"), dtype=torch.float32, device=eng.device),
           "features": torch.full((L, hops * hops + 2 * hops), float("nan"), dtype=torch.float32, device=eng.device)}
    N.check(N.lib().s3grl_sketch_pairs(eng._ctx, n, hops, P, p, N.ptr(mh), N.ptr(hl), N.ptr(lc), C, N.ptr(l_d), L,
                                       *(N.ptr(out[k]) if k in want else None for k in out)), "s3grl_sketch_pairs")
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in out.items()}


def _abi_ball_sizes(hl, p):
    from s3grl_amd import _native as N
    from s3grl_amd import sketch as S

    eng = _engine()
    _, C, lc = S.hll_constants(p)
    lc = torch.as_tensor(lc).to(eng.device)
    out = torch.full(hl.shape[:2], float("nan"), dtype=torch.float32, device=eng.device)
    N.check(N.lib().s3grl_sketch_cardinality(eng._ctx, p, N.ptr(lc), C, N.ptr(hl), out.numel(), N.ptr(out)),
            "s3grl_sketch_cardinality")
    torch.cuda.synchronize()
    return _np(out)


def _check_everything(what, A, links, hops, P, p, seed=0):
    """tables, ball sizes and every link output, for `links` and for the reversed links, whose intersections and raw
    integers must be the exact transposes"""
    mh_ref, hl_ref = R.sketches(A, hops, P, p, seed)
    mh, hl = _abi_build(A, hops, P, p, seed)
    for i in range(hops + 1):
        _same(f"{what} minhash hop {i}", _np(mh[i]).view(np.uint32), mh_ref[i])
        _same(f"{what} hll hop {i}", _np(hl[i]), hl_ref[i])
    _same(f"{what} ball_sizes", _abi_ball_sizes(hl, p), R.ball_sizes(hl_ref, p))
    got = {}
    for order, ll in (("(u, v)", links), ("(v, u)", links[::-1].copy())):
        ref = R.link_outputs(mh_ref, hl_ref, ll, p)
        got[order] = _abi_pairs(mh, hl, p, ll)
        for name in ("match", "T", "z", "intersections", "features"):
            _same(f"{what} {order} {name}", got[order][name], ref[name])
        assert not np.isnan(got[order]["features"]).any() and not np.isnan(got[order]["intersections"]).any()
    for name in ("match", "T", "z", "intersections"):
        assert np.array_equal(got["(v, u)"][name].view(np.uint8),
                              np.ascontiguousarray(got["(u, v)"][name].transpose(0, 2, 1)).view(np.uint8)), name
    return mh, hl, got["(u, v)"]


@lru_cache(maxsize=None)
def _graphs():
    """{name: (A, links)}: the comb (row lengths 0, 1, 2, 63, 64, 65, 127, 128, 129, 200), directed graphs with sinks
    and orphans, one node with a self-loop, and the 600-key hub with an isolated node and self-loops"""
    c = HC.comb_graph()
    out = {"comb": (c.A_int, c.links)}
    for n in (1, 17, 1041):
        g = HC.sink_graph(n)
        out[f"sink{n}"] = (g.A, HC.links_of(HC.sink_sources(g), n, per_source=3))
    out["hub"] = K.hub_graph()
    return out


# ---- bit-equality at every lane layout --------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"P{s[0]}p{s[1]}")
@pytest.mark.parametrize("hops", HOPS)
def test_tables_and_link_outputs_equal_the_restatement(hops, shape):
    P, p = shape
    for name, (A, links) in _graphs().items():
        _check_everything(f"{name} hops {hops} P {P} p {p}", A, links, hops, P, p, seed=hops * 1000 + P)


def test_split_rows_and_their_neighbours():
    """The hub graph at the defaults: rows of 600 and 260 keys go through the four-wavefront split, their workgroup's
    other rows (an empty row, a self-loop) through the one-wavefront path of the same workgroup."""
    A, links = K.hub_graph()
    assert np.diff(A.indptr)[:5].tolist() == [600, 260, 0, 1, 3] and A[3, 3] == 1 and A[:, 2].nnz == 0
    mh, hl, _ = _check_everything("hub defaults", A, links, 2, 128, 8)
    mh = _np(mh)
    assert np.array_equal(mh[0, 2], mh[1, 2]) and np.array_equal(mh[0, 2], mh[2, 2])      # a row without keys copies
    assert np.array_equal(mh[0, 3], mh[2, 3])                                              # a lone self-loop too
    assert np.array_equal(_np(hl)[0, 2], _np(hl)[2, 2])


@pytest.mark.parametrize("n,deg", ((300, 4), (3000, 6)))
def test_random_symmetric_graphs_at_the_defaults(n, deg):
    A, links = K.accuracy_case(n, deg)
    _check_everything(f"random {n}", A, links, 2, 128, 8)


def test_the_order_of_the_inclusion_exclusion_shows_and_holds():
    """`order_case`: links on which a reordered inclusion-exclusion differs in fp32 (the host test asserts that)."""
    A, links, hops, P, p = K.order_case()
    _, _, got = _check_everything("order case", A, links, hops, P, p)
    mh, hl = R.sketches(A, hops, P, p, 0)
    other = R.link_outputs(mh, hl, links, p, fault="ie_order")["features"]
    differ = int(np.count_nonzero(got["features"].view(np.uint32) != other.view(np.uint32)))
    print(f"[sketch] order case: {differ} features differ from the reordered sum")
    assert differ > 0


# ---- link lists -------------------------------------------------------------------------------------------------

def test_link_list_edges():
    """u == v, repeated links, L = 0, L = 1 and L no multiple of the four wavefronts of a workgroup."""
    A, _ = K.hub_graph()
    mh_ref, hl_ref = R.sketches(A, 2, 128, 8, 0)
    mh, hl = _abi_build(A, 2, 128, 8)
    base = np.array([[0, 0, 7, 7, 7, 1, 2, 3, 899, 0, 5], [0, 1, 7, 9, 9, 0, 2, 3, 899, 0, 6]], dtype=np.int64)
    for L in (1, 2, 3, 5, 11):
        links = base[:, :L]
        ref, got = R.link_outputs(mh_ref, hl_ref, links, 8), _abi_pairs(mh, hl, 8, links)
        for name in ref:
            _same(f"L = {L} {name}", got[name], ref[name])
    got = _abi_pairs(mh, hl, 8, base)
    for name in got:
        assert np.array_equal(got[name][3].view(np.uint8), got[name][4].view(np.uint8)), name      # a repeated link
        assert np.array_equal(got[name][0].view(np.uint8), got[name][9].view(np.uint8)), name
    # u == v: the diagonal of I is the ball itself, match is num_perm there
    assert np.all(got["match"][0].diagonal() == 128) and np.all(got["match"][2].diagonal() == 128)
    balls = _abi_ball_sizes(hl, 8)
    assert np.array_equal(got["intersections"][2].diagonal(), balls[:, 7])
    # only the outputs asked for are written
    some = _abi_pairs(mh, hl, 8, base, want=("features",))
    assert np.all(some["match"] == -1) and np.all(some["T"] == -1) and np.isnan(some["intersections"]).all()
    assert np.array_equal(some["features"].view(np.uint8), got["features"].view(np.uint8))
    # L = 0: the ABI touches nothing, the object returns empty tensors of the right shapes
    empty = _abi_pairs(mh, hl, 8, np.zeros((2, 0), dtype=np.int64))
    assert empty["features"].shape == (0, 8) and empty["intersections"].shape == (0, 3, 3)
    from s3grl_amd import sketch as S

    sk = S.SketchGraph(A)
    try:
        assert tuple(sk.features(np.zeros((2, 0), dtype=np.int64)).shape) == (0, 8)
        assert tuple(sk.intersections(torch.zeros((2, 0), dtype=torch.long)).shape) == (0, 3, 3)
        assert [tuple(t.shape) for t in sk.raw(np.zeros((2, 0), dtype=np.int64))] == [(0, 3, 3)] * 3
    finally:
        sk.close()


def test_bad_ids_are_refused_before_any_gpu_work():
    from s3grl_amd import sketch as S

    A, _ = K.hub_graph()
    mh, hl = _abi_build(A, 1, 64, 7)
    for bad in ([[0, 900], [1, 0]], [[0, -1], [1, 2]]):
        with pytest.raises(ValueError):
            _abi_pairs(mh, hl, 7, np.array(bad))
    sk = S.SketchGraph(A, hops=1, num_perm=64, hll_p=7)
    try:
        for bad in ([[0, 900], [1, 0]], [[0, -1], [1, 2]], [[0, 1, 2]]):
            for method in (sk.features, sk.intersections, sk.raw):
                with pytest.raises(ValueError):
                    method(np.array(bad))
    finally:
        sk.close()
    with pytest.raises(RuntimeError, match="closed"):
        sk.features(np.array([[0], [1]]))
    with pytest.raises(RuntimeError, match="closed"):
        sk.ball_sizes()


# ---- the object and determinism ---------------------------------------------------------------------------------

def test_the_object_equals_the_abi_and_is_deterministic():
    from s3grl_amd import sketch as S

    A, links = K.accuracy_case(300, 4)
    mh, hl = _abi_build(A, 2, 128, 8, seed=5)
    ref = _abi_pairs(mh, hl, 8, links)
    a, b, c = S.SketchGraph(A, seed=5), S.SketchGraph(A, seed=5), S.SketchGraph(A, seed=6)
    try:
        assert a.minhash.dtype == torch.int32 and tuple(a.minhash.shape) == (3, 300, 128)
        assert a.hll.dtype == torch.uint8 and tuple(a.hll.shape) == (3, 300, 256)
        assert torch.equal(a.minhash, mh) and torch.equal(a.hll, hl)
        assert torch.equal(a.minhash, b.minhash) and torch.equal(a.hll, b.hll)              # one seed, one table
        assert not torch.equal(a.minhash, c.minhash) and not torch.equal(a.hll, c.hll)      # another seed, another
        _same("object ball_sizes", _np(a.ball_sizes()), _abi_ball_sizes(hl, 8))
        match, T, z = a.raw(links)
        for name, got in (("match", match), ("T", T), ("z", z), ("intersections", a.intersections(links)),
                          ("features", a.features(torch.as_tensor(links)))):
            _same(f"object {name}", _np(got), ref[name])
        perm = np.random.default_rng(3).permutation(links.shape[1])                        # a permuted list permutes
        _same("permuted features", _np(a.features(links[:, perm])), ref["features"][perm])
        _same("permuted intersections", _np(a.intersections(links[:, perm])), ref["intersections"][perm])
        _same("second call", _np(b.features(links)), ref["features"])
        assert a in a.engine._children
    finally:
        for sk in (a, b, c):
            sk.close()


# ---- end to end -------------------------------------------------------------------------------------------------

def test_run_buddy_on_usair_learns_and_beats_chance():
    """The packaged USAir topology, no features, 8 epochs: every step's loss finite, the last epoch's mean below the
    first's, and the test AUC above 0.5 by more than five standard deviations of a chance ranking,
    5·√((n⁺ + n⁻ + 1) / (12·n⁺·n⁻)).  The AUC itself is only printed."""
    from s3grl_amd import sketch as S
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    split = W.edge_split(n, e, seed=0)
    history, epochs, batch = [], 8, 1024
    res = S.run_buddy(split, hops=2, epochs=epochs, lr=0.01, seed=1, batch_size=batch, history=history)
    n_train = split.links["train"][0].shape[1] + split.links["train"][1].shape[1]
    steps = -(-n_train // batch)
    assert len(history) == epochs * steps and np.all(np.isfinite(history))
    first, last = float(np.mean(history[:steps])), float(np.mean(history[-steps:]))
    n_pos, n_neg = split.links["test"][0].shape[1], split.links["test"][1].shape[1]
    margin = 5.0 * np.sqrt((n_pos + n_neg + 1) / (12.0 * n_pos * n_neg))
    print(f"[sketch] run_buddy USAir: loss {first:.4f} -> {last:.4f}, AUC val {res['AUC'][0]:.4f} test "
          f"{res['AUC'][1]:.4f} (chance + {margin:.4f}), AP test {res['AP'][1]:.4f}")
    assert last < first
    assert res["AUC"][1] > 0.5 + margin
    assert set(res) == {"AUC", "AP"} and all(len(v) == 2 for v in res.values())
