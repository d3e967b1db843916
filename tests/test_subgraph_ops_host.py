"""Host-side checks (no GPU) of tests/subgraph_op_cases.py: the sweeps reach every compiled instance of the subgraph
operators' kernels, the small graph has the shapes it promises, and the restatement run in float32 on the sweep's own
inputs stays inside every bound that test_gpu_subgraph_ops.py holds the kernels to."""
import numpy as np
import pytest
import torch

import subgraph_op_cases as cases
from mpnn_reference import aggregate_mean, aggregate_mean_t, aggregate_sum, aggregate_sum_t, in_degree, segment_mean
from seal_nn_reference import gcn_norm, propagate


def test_aggregation_sweep_reaches_every_instance():
    paths = {H: cases.agg_path(H) for H in cases.AGG_H}
    pairs = {p[:2] for p in paths.values()}
    assert pairs == {(v, l) for v in (1, 4) for l in (1, 2, 4, 8, 16, 32, 64)}            # all 14 (VEC, LPN)
    for vec in (1, 4):
        assert {p[2] for p in paths.values() if p[:2] == (vec, 64)} == {1, 2}             # the channel loop's 2nd trip
    assert paths[16] == (4, 4, 1) and paths[256] == (4, 64, 1)                           # groups filled exactly
    assert paths[3] == (1, 4, 1) and paths[12] == (4, 4, 1)                              # groups with idle lanes
    assert cases.agg_rows_per_block(1) == 256 and cases.agg_rows_per_block(256) == 4
    # the restatement itself, by hand: H = 260 is 65 float4 columns on 64 lanes
    assert cases.agg_path(260) == (4, 64, 2) and cases.agg_path(65) == (1, 64, 2) and cases.agg_path(64) == (4, 16, 1)


def test_segment_mean_sweep_reaches_every_instance():
    paths = [cases.seg_path(W) for W in cases.SEG_W]
    assert {p[0] for p in paths} == {1, 2, 4, 8, 16, 32, 64}                              # all 7 CL
    assert {p[1] for p in paths if p[0] == 64} >= {1, 2, 4}                               # one and several tiles
    assert {p[2] for p in paths} == {"divides", "wave"}
    assert cases.seg_path(512) == (64, 8, "wave") and cases.seg_path(128) == (64, 2, "divides")
    chunks = [-(-s // cases.SEG_CHUNK) for s in cases.SEG_SIZES]
    assert {1, 2, 3} <= set(chunks) and 0 in cases.SEG_SIZES[1:-1]
    assert cases.SEG_CHUNK in cases.SEG_SIZES and cases.SEG_CHUNK + 1 in cases.SEG_SIZES
    assert max(cases.SEG_SIZES[:cases.SEG_PREFIX]) == cases.SEG_CHUNK                     # the chunks == 1 launch
    # a second trip of the 4-wide row loop for the widest slices: CL = 64 has 4 slices, so 16 rows a trip
    assert max(cases.SEG_SIZES) > 2 * 16


def test_copy_sweep_reaches_both_paths_at_one_trip_and_two():
    paths = {cases.copy_path(D) for D in cases.COPY_D}
    assert {("float4", 1), ("float4", 2), ("dword", 1), ("dword", 2)} <= paths
    centre = {cases.copy_path(H, "centre") for H in cases.POOL_H}
    assert {("float4", 1), ("float4", 2), ("dword", 1), ("dword", 2)} <= centre


def test_small_graph_shapes():
    n, arcs = cases.small_graph()
    src, dst = arcs[:, 0], arcs[:, 1]
    d_in, d_out = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    assert n == 60 and sorted(set(d_in)) == list(range(10)) and sorted(set(d_out)) == list(range(10))
    assert int(((d_in == 0) & (d_out == 0)).sum()) == 2                                   # two isolated nodes
    assert ((d_in == 0) & (d_out > 0)).any() and ((d_out == 0) & (d_in > 0)).any()
    assert (src == dst).any()                                                             # input self-loops
    assert len(np.unique(arcs, axis=0)) < len(arcs)                                       # duplicated arcs
    pairs = set(map(tuple, arcs))
    assert any((v, u) not in pairs for u, v in pairs)                                     # really directed
    w = cases.arc_weights(arcs)
    assert set(w.tolist()) == {1.0, 2.0, 3.0, 4.0}
    A = cases.small_graph_csr()
    assert A.nnz == len(pairs) and set(A.data.tolist()) == {1, 2, 3, 4}
    li = cases.small_links()
    assert li.shape == (2, 30) and (li[0] != li[1]).all() and li.max() < 58
    assert cases.edgeless_graph()[1].shape == (0, 2)
    for m in (1, 3, 4, 5, 255, 256, 257):
        k, a = cases.ring_graph(m)
        assert k == m and a.max() == m - 1 and set(a[:, 0]) == set(range(m))


def _inputs(n, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, H), generator=g), torch.randn((n, H), generator=g), torch.randn(H, generator=g)


def _graphs():
    n, arcs = cases.small_graph()
    yield n, arcs, None
    yield n, arcs, cases.arc_weights(arcs)
    yield cases.edgeless_graph() + (None,)
    for m in (1, 5):
        yield cases.ring_graph(m) + (None,)


def test_fp32_restatement_stays_inside_the_aggregation_bounds():
    worst = 0.0
    for n, arcs, _ in _graphs():
        src, dst = torch.as_tensor(arcs[:, 0]), torch.as_tensor(arcs[:, 1])
        for H in cases.AGG_H:
            h, gout, _ = _inputs(n, H, H)
            for mode in ("sum", "mean"):
                fwd, bwd = (aggregate_mean, aggregate_mean_t) if mode == "mean" else (aggregate_sum, aggregate_sum_t)
                for self_coef in (0.0, 1.25):
                    ref, bound, ref_g, bound_g = cases.aggregate_reference(h.double(), gout.double(), src, dst, mode,
                                                                           self_coef)
                    out = self_coef * h + fwd(h, src, dst)
                    gh = self_coef * gout + bwd(gout, src, dst)
                    assert out.dtype == torch.float32 and gh.dtype == torch.float32
                    worst = max(worst, cases.ratio(out, ref, bound), cases.ratio(gh, ref_g, bound_g))
    print(f"[subgraph ops] raw aggregation, restatement in fp32: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


def test_fp32_restatement_stays_inside_the_gcn_bound():
    worst = 0.0
    for n, arcs, w in _graphs():
        ei = torch.as_tensor(arcs.T.copy())
        wt = torch.as_tensor(w) if w is not None else None
        src, dst, coef = gcn_norm(ei, n, wt)
        s32, d32, c32 = gcn_norm(ei, n, wt, dtype=torch.float32)
        assert c32.dtype == torch.float32 and torch.equal(s32, src) and torch.equal(d32, dst)
        assert float(in_degree(dst, n).min()) >= 1                                        # every node has its loop
        for H in cases.AGG_H:
            h, gout, bias = _inputs(n, H, 100 + H)
            for b in (bias, None):
                ref, bound, ref_g, bound_g = cases.gcn_reference(h.double(), gout.double(),
                                                                 b.double() if b is not None else None, src, dst, coef)
                out = propagate(h, src, dst, c32)
                out = out + b if b is not None else out
                gh = propagate(gout, dst, src, c32)
                assert out.dtype == torch.float32
                worst = max(worst, cases.ratio(out, ref, bound), cases.ratio(gh, ref_g, bound_g))
    print(f"[subgraph ops] GCN propagation, restatement in fp32: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("W", [1, 5, 65])
def test_fp32_restatement_stays_inside_the_segment_mean_bound(W):
    ptr = cases.segments(cases.SEG_SIZES)
    g = torch.Generator().manual_seed(W)
    x = torch.randn((int(ptr[-1]), W), generator=g)
    gout = torch.randn((ptr.numel() - 1, W), generator=g)
    ref, bound, ref_g, bound_g = cases.segment_mean_reference(x.double(), gout.double(), ptr)
    out = segment_mean(x, ptr)
    graph = torch.repeat_interleave(torch.arange(ptr.numel() - 1), ptr.diff())
    gx = (gout / ptr.diff().clamp(min=1).float()[:, None])[graph]
    assert out.dtype == torch.float32 and gx.dtype == torch.float32
    worst = max(cases.ratio(out, ref, bound), cases.ratio(gx, ref_g, bound_g))
    print(f"[subgraph ops] segment mean W = {W}, restatement in fp32: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst
    assert bool((out[2] == 0).all()) and bool((out[9] == 0).all())                       # the empty graphs


@pytest.mark.parametrize("mode", ["", "mean", "sum"])
def test_fp32_restatement_stays_inside_the_centre_pool_bound(mode):
    rp = cases.segments([2, 5, 2, 3, 9, 2, 4])
    worst = 0.0
    for H in cases.POOL_H:
        g = torch.Generator().manual_seed(H)
        h = torch.randn((int(rp[-1]), H), generator=g)
        ref = cases.centre_pool_torch(h.double(), rp, mode)
        worst = max(worst, cases.ratio(cases.centre_pool_torch(h, rp, mode), ref,
                                       cases.centre_pool_bound(h.double(), rp, mode)))
    print(f"[subgraph ops] centre pool {mode or 'none'}, restatement in fp32: worst error / bound {worst:.3f}")
    assert worst <= 1.0, worst


def test_aligned16_keeps_aligned_tensors_and_copies_the_rest():
    from s3grl_amd import _native

    buf = torch.zeros(64)
    assert buf.data_ptr() % 16 == 0
    assert _native.aligned16(buf) is buf
    off = buf[1:37].view(9, 4)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    fixed = _native.aligned16(off)
    assert fixed is not off and fixed.data_ptr() % 16 == 0 and torch.equal(fixed, off)
