"""Test infrastructure: the cases of tests/test_subgraph_ops_host.py and tests/test_gpu_subgraph_ops.py.  It restates
how the four subgraph operators pick a kernel instance from a width (csrc/s3grl_propagate.hip launch_vec / launch_agg,
s3grl_mpnn.hip, s3grl_seal_nn.hip, s3grl_pool.hip), holds the width sweeps that reach every instance, one small
directed graph that covers every remainder of the unrolled neighbour walk, and the forward-error bounds, each stated
from the fp64 restatement alone (seal_nn_reference.py, mpnn_reference.py).  Imports no GPU code; everything here runs
on the device of its inputs.

Bounds (u = 2^-24; where a bound is 0 the result must be exact):
  raw aggregation, a row with d entries   (d + 3) · u · (|self_coef · h_i| + Σ_e |s(e) · h_j|)       test_gpu_mpnn.py
  segment mean, a graph of n rows         (n + 2) · u · Σ|x| / n;  backward  u · |grad_out / n|       test_gpu_mpnn.py
  GCN, an output element with d CSR entries (the loop included)
                                          (d + 12) · u · (Σ_e |coef_e · h_j| + |bias|)
      relative to Σ|term|, to first order: dinv = 1 / sqrtf(deg) costs at most 2u for sqrtf and 2u for the reciprocal,
      and coef holds dinv twice: 8u; coef's two products dinv[j] · w · dinv[i]: 2u; the product coef · h_j of every
      term: u; the d adds of the terms, each at most u times a partial sum that Σ|term| bounds: d·u; the bias add: u;
      together d + 12.  Degree sums are exact: the weights are small integers.
  centre pool                             forward: u · |h_src · h_dst|, and (m + 2) · u · s · Σ_e |h_e| for the pooled
      half of a link with m further rows (m - 1 adds, the scale s = 1 / m and its product); backward: 2u · |ref|
      (one product, or the scale and its product), so the gradient rows of mode "none" past the second are exact zeros
"""
import numpy as np
import torch

from mpnn_reference import (aggregate_mean, aggregate_mean_t, aggregate_sum, aggregate_sum_t, in_degree,
                            segment_mean)
from seal_nn_reference import propagate

U = 2.0 ** -24

# ---- which instance a width runs -----------------------------------------------------------------------------------
AGG_BLOCK_WAVES = 4          # kAggWaves
SEG_CHUNK = 2048             # kSegChunk
SORT_BLOCK = 256             # kNnBlock


def agg_path(H):
    """(VEC, LPN, trips) of nbr_agg_kernel at H channels: float4 when H % 4 == 0, LPN the smallest power of two >=
    H / VEC capped at 64, trips the turns of the channel loop of a group's first lane."""
    vec = 4 if H % 4 == 0 else 1
    cols = H // vec
    lpn = 1
    while lpn < cols and lpn < 64:
        lpn <<= 1
    return vec, lpn, -(-cols // lpn)


def agg_rows_per_block(H):
    """Rows one workgroup of nbr_agg_kernel takes at H channels."""
    return AGG_BLOCK_WAVES * 64 // agg_path(H)[1]


def seg_path(W):
    """(CL, column tiles, "divides" | "wave") of the segment mean at width W: CL column lanes (the smallest power of
    two >= W, capped at 64), ceil(W / CL) tiles, and the backward's branch (256 % W == 0 or a wavefront per row)."""
    cl = 1
    while cl < W and cl < 64:
        cl <<= 1
    return cl, -(-W // cl), "divides" if 256 % W == 0 else "wave"


def copy_path(D, op="sortpool"):
    """("float4" | "dword", trips) of a row copy of D floats by one wavefront: SortPool's forward and backward copy
    16 bytes per lane when D % 4 == 0 (256 floats a trip), else 4 (64 floats a trip); centre pool's forward
    (op="centre") gives every lane four neighbouring floats on either path (256 a trip)."""
    kind = "float4" if D % 4 == 0 else "dword"
    per_trip = 256 if kind == "float4" or op == "centre" else 64
    return kind, -(-D // per_trip)


# non-powers of two leave idle lanes in a group; 16 and 256 fill theirs exactly
AGG_H = [1, 2, 3, 5, 9, 17, 33, 65, 4, 8, 12, 20, 36, 68, 132, 260, 16, 256]
SEG_W = [1, 2, 3, 5, 9, 17, 33, 65, 128, 256, 512]
COPY_D = [1, 3, 4, 8, 97, 257, 260]
POOL_H = [1, 3, 4, 8, 257, 260]
SEG_SIZES = [1, 2, 0, 63, 64, 65, 769, 2048, 2049, 0, 4097, 3]     # one chunk exactly, two, three; empty graphs
SEG_PREFIX = 8                                                       # SEG_SIZES[:8]: no graph longer than a chunk


# ---- graphs ----------------------------------------------------------------------------------------------------
SMALL_N = 60
_ACTIVE = 58                 # nodes 58 and 59 are isolated


def small_graph():
    """(n, arcs [E, 2] int64, src -> dst): 60 nodes, node i < 58 with in-degree i % 10 and out-degree (57 - i) % 10,
    so every in- and out-degree 0..9 (every remainder of the 4-wide walk, and the empty row, in both CSRs), nodes
    without in-arcs that have out-arcs and the reverse, two isolated nodes; the stubs are paired by a fixed stride,
    which leaves input self-loops and duplicated arcs (test_subgraph_ops_host.py asserts all of it)."""
    heads = np.repeat(np.arange(_ACTIVE), np.arange(_ACTIVE) % 10)
    tails = np.repeat(np.arange(_ACTIVE), (57 - np.arange(_ACTIVE)) % 10)
    E = heads.size
    assert tails.size == E
    t = (np.arange(E) * 100 + 7) % E                 # gcd(100, 253) = 1: a permutation of the out-stubs
    return SMALL_N, np.stack([tails[t], heads], 1).astype(np.int64)


def arc_weights(arcs):
    """Integer weights 1..4, a function of the pair (duplicates of an arc agree), float32."""
    return (1 + (3 * arcs[:, 0] + 5 * arcs[:, 1]) % 4).astype(np.float32)


def edgeless_graph():
    return SMALL_N, np.zeros((0, 2), dtype=np.int64)


def small_graph_csr(weighted=True):
    """The small graph as the scipy CSR A[u, v] = w(u, v) that enclosing_subgraphs takes: one entry per distinct
    arc, int64 values 1..4 (or ones)."""
    import scipy.sparse as ssp

    n, arcs = small_graph()
    pairs = np.unique(arcs, axis=0)
    w = arc_weights(pairs).astype(np.int64) if weighted else np.ones(len(pairs), dtype=np.int64)
    return ssp.csr_matrix((w, (pairs[:, 0], pairs[:, 1])), shape=(n, n))


def small_links(count=30):
    """[2, count] links between distinct active nodes of the small graph."""
    s = np.arange(count) * 2 % _ACTIVE
    d = (s * 7 + 3) % _ACTIVE
    d = np.where(d == s, (d + 1) % _ACTIVE, d)
    return np.stack([s, d]).astype(np.int64)


def ring_graph(n):
    """(n, arcs) of exactly n nodes: i -> i + 1 and i -> 3i + 1 (mod n); a graph of one node is one self-loop."""
    i = np.arange(n)
    return n, np.concatenate([np.stack([i, (i + 1) % n], 1), np.stack([i, (3 * i + 1) % n], 1)]).astype(np.int64)


def segments(sizes):
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.as_tensor(sizes), 0)
    return ptr


# ---- references and bounds (fp64, on the inputs' device) ---------------------------------------------------------
def ratio(got, ref, bound):
    """max |got - ref| / bound; where the bound is 0 the result must be exact."""
    err = (got.double() - ref).abs()
    zero = bound == 0
    assert bool((err[zero] == 0).all()), "an element with a zero bound is not exact"
    return float((err[~zero] / bound[~zero]).max()) if bool((~zero).any()) else 0.0


def aggregate_reference(h, gout, src, dst, mode, self_coef):
    """(ref, bound, ref_grad, bound_grad) of aggregate(h, ., mode, self_coef) and of its backward from gout; fp64."""
    n = h.shape[0]
    fwd, bwd = (aggregate_mean, aggregate_mean_t) if mode == "mean" else (aggregate_sum, aggregate_sum_t)
    d_in, d_out = in_degree(dst, n)[:, None], in_degree(src, n)[:, None]
    ref = self_coef * h + fwd(h, src, dst)
    bound = (d_in + 3) * U * ((self_coef * h).abs() + fwd(h.abs(), src, dst))
    ref_g = self_coef * gout + bwd(gout, src, dst)
    bound_g = (d_out + 3) * U * ((self_coef * gout).abs() + bwd(gout.abs(), src, dst))
    return ref, bound, ref_g, bound_g


def gcn_reference(h, gout, bias, src, dst, coef):
    """(ref, bound, ref_grad, bound_grad) of GCN propagation over the arcs (src, dst, coef) of gcn_norm (loops
    included) and of its backward from gout; bias fp64 [H] or None."""
    n = h.shape[0]
    d_in, d_out = in_degree(dst, n)[:, None], in_degree(src, n)[:, None]
    b = bias if bias is not None else torch.zeros(h.shape[1], dtype=h.dtype, device=h.device)
    ref = propagate(h, src, dst, coef) + b
    bound = (d_in + 12) * U * (propagate(h.abs(), src, dst, coef.abs()) + b.abs())
    ref_g = propagate(gout, dst, src, coef)
    bound_g = (d_out + 12) * U * propagate(gout.abs(), dst, src, coef.abs())
    return ref, bound, ref_g, bound_g


def segment_mean_reference(x, gout, ptr):
    """(ref, bound, ref_grad, bound_grad) of the segment mean of x over ptr and of its backward from gout; fp64."""
    ptr = ptr.to(x.device)
    n = ptr.diff().double()[:, None]
    ref = segment_mean(x, ptr)
    bound = (n + 2) * U * segment_mean(x.abs(), ptr)
    graph = torch.repeat_interleave(torch.arange(n.shape[0], device=x.device), ptr.diff())
    ref_g = (gout / n.clamp(min=1))[graph]
    return ref, bound, ref_g, U * ref_g.abs()


def centre_pool_torch(h, row_ptr, mode):
    """The formula of reference models.py:339-369 in torch (differentiable): [h_src · h_dst | pool of the further
    rows], mode "" (no pool), "mean" or "sum"; links without further rows pool to zeros."""
    rp = [int(v) for v in row_ptr]
    c = torch.as_tensor(rp[:-1], device=h.device)
    parts = [h[c] * h[c + 1]]
    if mode:
        pooled = []
        for b in range(len(rp) - 1):
            extra = h[rp[b] + 2: rp[b + 1]]
            pooled.append(extra.sum(0) if mode == "sum" or len(extra) == 0 else extra.mean(0))
        parts.append(torch.stack(pooled))
    return torch.cat(parts, -1)


def centre_pool_bound(h, row_ptr, mode):
    """The forward bound of centre pool (this module's docstring) for h fp64."""
    rp = [int(v) for v in row_ptr]
    c = torch.as_tensor(rp[:-1], device=h.device)
    parts = [U * (h[c] * h[c + 1]).abs()]
    if mode:
        pooled = []
        for b in range(len(rp) - 1):
            extra = h[rp[b] + 2: rp[b + 1]].abs()
            m = len(extra)
            pooled.append((m + 2) * U * extra.sum(0) / (m if mode == "mean" and m else 1))
        parts.append(torch.stack(pooled))
    return torch.cat(parts, -1)
