"""CPU checks of the subgraph-sketch restatement (tests/sketch_reference.py): the definitions (hash,
rank, linear-counting table, inclusion-exclusion on exact sets), its accuracy against the true sets, the named faults
against the bit-equality the GPU test uses, the argument checks that refuse before any GPU work, and the public
surface.

Accuracy, on two seeded random symmetric graphs (300 nodes at mean degree 4, 3 000 nodes at mean degree 6), hops 2,
P 128, p 8, 2 000 links of which half are edges.  Both are conditions:
 (i)  per hop, the mean relative error of the ball sizes is at most HyperLogLog's standard error 1.04/√m = 0.065;
 (ii) per (i, j), at most 1 % of the links have |I_ij − exact| > 4·sd, sd = √(J(1−J)/P)·|∪| + (1.04/√m)·|∩| from the
      exact sets: the binomial standard deviation of the matching slots scaled to the union, plus the union
      estimate's own error carried into the product."""
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as ssp

import sketch_cases as K
import sketch_reference as R

REPO = Path(__file__).resolve().parent.parent
HOPS, P, HLL_P = 2, 128, 8


@lru_cache(maxsize=None)
def _case(n, mean_degree):
    """graph, its 2 000 links, the restatement and the true sets"""
    A, links = K.accuracy_case(n, mean_degree)
    mh, hl = R.sketches(A, HOPS, P, HLL_P, seed=0)
    return A, links, mh, hl, R.exact_counts(A, links, HOPS)


# ---- definitions -------------------------------------------------------------------------------------------------

def test_hash_against_hand_computed_values():
    # murmur3's finaliser: fmix32(0) = 0; fmix32(1) and fmix32(0xFFFFFFFF) worked through by hand below
    assert int(R.fmix32(0)) == 0

    def by_hand(h):
        h ^= h >> 16
        h = h * 0x85EBCA6B % 2 ** 32
        h ^= h >> 13
        h = h * 0xC2B2AE35 % 2 ** 32
        return h ^ (h >> 16)

    assert by_hand(1) == 0x514E28B7 and int(R.fmix32(1)) == 0x514E28B7
    assert by_hand(0xFFFFFFFF) == 0x81F16F39 and int(R.fmix32(0xFFFFFFFF)) == 0x81F16F39
    for seed, s, v in ((0, 0, 0), (0, 5, 7), (12345, 128, 2 ** 24 - 1), (2 ** 32 - 1, 512, 3)):
        c = by_hand((seed + s * 0x27D4EB2F) % 2 ** 32)
        want = by_hand((v * 0x9E3779B1 + c) % 2 ** 32)
        assert int(R.slot_constants(s + 1, seed)[s]) == c
        assert int(R.hashes([v], s + 1, seed)[0, s]) == want


@pytest.mark.parametrize("p", (7, 8, 9, 10))
def test_rank_edges(p):
    width = 32 - p
    assert int(R.rank(0, p)) == 33 - p                           # a zero field
    assert int(R.rank((1 << width) - 1, p)) == 1                 # all ones: no leading zero
    assert int(R.rank(1 << (width - 1), p)) == 1                 # top bit only
    assert int(R.rank(1, p)) == width                            # lowest bit only
    assert int(R.rank(1 << (width - 2), p)) == 2


@pytest.mark.parametrize("p", (7, 8, 9, 10))
def test_hop_zero_and_the_linear_counting_table(p):
    m, Rr, C, LC = R.constants(p)
    assert m == 1 << p and Rr == 33 - p and len(LC) == m + 1
    assert LC[m] == 0.0 and LC[1] == m * np.log(float(m)) and np.all(np.diff(LC[1:]) < 0)
    assert C == 0.7213 / (1.0 + 1.079 / m) * m * m * 2.0 ** Rr
    A = ssp.csr_matrix((5, 5))
    mh, hl = R.sketches(A, 1, 64, p, seed=3)
    assert np.array_equal(mh[0], R.hashes(np.arange(5), 64, 3)) and np.array_equal(mh[1], mh[0])
    assert np.all((hl[0] != 0).sum(axis=1) == 1) and np.array_equal(hl[1], hl[0])
    h = R.hashes(np.arange(5), 65, 3)[:, 64]
    assert np.array_equal(np.argmax(hl[0], axis=1), h >> np.uint32(32 - p))
    # one register set: T = (m - 1)·2^R + 2^(R - rank), z = m - 1, and the estimate of a single node is LC[m - 1] ≈ 1
    T, z = R.tz(hl[0], p)
    assert np.array_equal(z, np.full(5, m - 1))
    assert np.array_equal(T, (m - 1) * 2 ** Rr + 2 ** (Rr - hl[0].max(axis=1).astype(np.int64)))
    assert np.allclose(R.cardinality(hl[0], p), 1.0, atol=0.01)
    # the harmonic-mean branch: no zero register, every register 1 -> α·m²/(m/2) = 2·α·m
    full = np.ones((1, m), dtype=np.uint8)
    assert R.cardinality(full, p)[0] == C / float(m * 2 ** (Rr - 1))


@pytest.mark.parametrize("n,deg", ((300, 4), (3000, 6)))
def test_inclusion_exclusion_on_exact_intersections_gives_the_exact_counts(n, deg):
    _, links, _, _, ex = _case(n, deg)
    F = R.features(ex["inter"].astype(np.float64), ex["balls_u"].astype(np.float64), ex["balls_v"].astype(np.float64))
    assert np.array_equal(F, ex["features"])
    assert ex["features"].min() >= 0 and ex["features"][:, :HOPS * HOPS].sum() > 0


# ---- accuracy ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,deg", ((300, 4), (3000, 6)))
def test_ball_sizes_within_hyperloglog_standard_error(n, deg):
    A, _, _, hl, _ = _case(n, deg)
    every = np.stack([np.arange(n), np.arange(n)])
    exact = R.exact_counts(A, every, HOPS)["balls_u"].T          # [hops+1, N]
    est = R.ball_sizes(hl, HLL_P).astype(np.float64)
    for i in range(HOPS + 1):
        err = float(np.mean(np.abs(est[i] - exact[i]) / exact[i]))
        print(f"n {n} hop {i}: mean ball {exact[i].mean():.1f}, mean relative error {err:.4f}")
        assert err <= 1.04 / np.sqrt(1 << HLL_P)


@pytest.mark.parametrize("n,deg", ((300, 4), (3000, 6)))
def test_intersections_within_four_standard_deviations(n, deg):
    _, links, mh, hl, ex = _case(n, deg)
    I = R.intersections(*R.raw(mh, hl, links, HLL_P), P, HLL_P)
    inter, union = ex["inter"].astype(np.float64), ex["union"].astype(np.float64)
    J = inter / union
    sd = np.sqrt(J * (1.0 - J) / P) * union + 1.04 / np.sqrt(1 << HLL_P) * inter
    outside = np.abs(I - inter) > 4.0 * sd
    for i in range(HOPS + 1):
        for j in range(HOPS + 1):
            share = float(outside[:, i, j].mean())
            print(f"n {n} I_{i}{j}: mean exact {inter[:, i, j].mean():.2f}, share outside 4 sd {share:.4f}")
            assert share <= 0.01


# ---- the named faults leave the bit-equality -----------------------------------------------------------------------

def _outputs(case, fault):
    A, links, hops, num_perm, p = case
    mh, hl = R.sketches(A, hops, num_perm, p, seed=0, fault=fault)
    out = R.link_outputs(mh, hl, links, p, fault=fault)
    out.update(minhash=mh, hll=hl, ball_sizes=R.ball_sizes(hl, p))
    return out


@pytest.mark.parametrize("fault,where", (("min_without_self", ("minhash", "match", "intersections", "features")),
                                         # balls this small are counted by LC[z], which sees no rank: only the
                                         # registers and the raw T show it, which is why `raw` is compared
                                         ("rank_off_by_one", ("hll", "T")),
                                         ("match_short", ("match", "intersections", "features")),
                                         ("ie_order", ("features",))))
def test_named_faults_break_bit_equality(fault, where):
    """Each fault changes at least one entry of the arrays named, under the comparison the GPU test uses (equal
    bytes).  The order of the inclusion-exclusion shows in fp32 only on `order_case` (see there), which the GPU test
    therefore runs too."""
    assert fault in R.FAULTS
    case = K.order_case() if fault == "ie_order" else K.accuracy_case(300, 4) + (HOPS, P, HLL_P)
    good, bad = _outputs(case, None), _outputs(case, fault)
    for name in good:
        differ = int(np.sum(good[name].view(np.uint8) != bad[name].view(np.uint8)))
        print(f"{fault}: {name}: {differ} bytes differ")
        if name in where:
            assert differ != 0, f"{fault} leaves {name} bit-equal"
    again = _outputs(case, None)
    assert all(np.array_equal(good[k].view(np.uint8), again[k].view(np.uint8)) for k in good)


# ---- argument checks that need no device -------------------------------------------------------------------------

def test_parameter_envelope():
    from s3grl_amd import sketch as S

    assert S.check_params(1, 64, 7, 0) == (1, 64, 7, 0)
    assert S.check_params(np.int64(4), 512, 10, 2 ** 32 - 1) == (4, 512, 10, 2 ** 32 - 1)
    for bad in ((0, 128, 8, 0), (5, 128, 8, 0), (2, 0, 8, 0), (2, 32, 8, 0), (2, 96, 8, 0), (2, 576, 8, 0),
                (2, 128, 6, 0), (2, 128, 11, 0), (2, 128, 8, -1), (2, 128, 8, 2 ** 32), (2.0, 128, 8, 0),
                (2, 128.0, 8, 0), (True, 128, 8, 0), (2, 128, "8", 0), (2, 128, 8, None)):
        with pytest.raises(ValueError):
            S.check_params(*bad)
    A = ssp.csr_matrix(([1, 1], ([0, 1], [1, 0])), shape=(3, 3))
    for kw in (dict(hops=0), dict(hops=5), dict(num_perm=100), dict(hll_p=6), dict(hll_p=11), dict(seed=-1)):
        with pytest.raises(ValueError):
            S.SketchGraph(A, **kw)
        with pytest.raises(ValueError):
            S.run_buddy(None, **({"sketch_seed": -1} if "seed" in kw else kw))
    for kw in (dict(epochs=0), dict(lr=0.0), dict(batch_size=1)):
        with pytest.raises(ValueError):
            S.run_buddy(None, **kw)


def test_graph_envelope():
    from s3grl_amd import sketch as S

    with pytest.raises(ValueError, match="square"):
        S.SketchGraph(ssp.csr_matrix((3, 4)))
    with pytest.raises(ValueError, match="2\\^24"):
        S.SketchGraph(ssp.csr_matrix((0, 0)))
    with pytest.raises(ValueError, match="2\\^24"):
        S.SketchGraph(ssp.csr_matrix(((1 << 24) + 1, (1 << 24) + 1)))
    A = S.check_graph(ssp.csr_matrix(([2.0, 0.0, 1.0, 1.0], ([0, 0, 1, 1], [1, 2, 0, 0])), shape=(3, 3)))
    assert A.nnz == 2 and A.indices.tolist() == [1, 0]          # explicit zeros dropped, duplicates merged


def test_no_cpu_fallback_and_bad_ids():
    from s3grl_amd import sketch as S
    from s3grl_amd.heuristics import check_links

    A = ssp.csr_matrix(([1, 1], ([0, 1], [1, 0])), shape=(3, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.SketchGraph(A, device="cpu")
    shell = object.__new__(S.SketchGraph)                        # a closed object: the id checks come first
    shell.num_nodes, shell.hops, shell.minhash = 3, 2, None
    for method in (shell.features, shell.intersections, shell.raw):
        with pytest.raises(RuntimeError, match="closed"):
            method(np.array([[0], [1]]))
    for bad in ([[0, 3], [1, 0]], [[0, -1], [1, 2]], [[0, 1, 2]], [[0.5], [1.0]]):
        with pytest.raises(ValueError):
            check_links(np.array(bad), 3)


def test_buddy_twin_layout():
    import torch

    from s3grl_amd import sketch as S

    for bad in (dict(num_features=-1, hops=2), dict(num_features=0, hops=0), dict(num_features=0, hops=5),
                dict(num_features=0, hops=2, hidden=0), dict(num_features=0, hops=2, dropout=1.0)):
        with pytest.raises(ValueError):
            S.BuddyTwin(**bad)
    torch.manual_seed(0)
    plain = S.BuddyTwin(0, 2, hidden=8)
    assert plain.label_lin.in_features == 8 and not hasattr(plain, "feat_lin") and plain.lin.in_features == 8
    assert plain(torch.randn(5, 8)).shape == (5,)
    both = S.BuddyTwin(6, 3, hidden=4, dropout=0.0).eval()
    assert both.label_lin.in_features == 15 and both.feat_lin.in_features == 6 and both.lin.in_features == 8
    s, xu, xv = torch.randn(7, 15), torch.randn(7, 6), torch.randn(7, 6)
    assert both(s, xu, xv).shape == (7,) and torch.equal(both(s, xu, xv), both(s, xv, xu))   # x_u ⊙ x_v commutes


# ---- the public surface: fails without the feature ----------------------------------------------------------------

def test_sketch_calls_are_declared_exported_and_reexported():
    import s3grl_amd
    from s3grl_amd import _native
    from s3grl_amd import sketch as S

    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_sketch_[a-z_]+)\s*\(", header))
    assert declared == {"s3grl_sketch_build", "s3grl_sketch_cardinality", "s3grl_sketch_pairs"}
    assert declared <= set(_native.SYMBOLS)
    assert "s3grl_sketch.hip" in __import__("__graft_entry__").SOURCES
    assert re.search(r"#define\s+S3GRL_SKETCH_MAX_HOPS\s+4\b", header) and S.MAX_HOPS == 4 and S.MAX_NODES == 1 << 24
    lib = _native.lib()
    for name in declared:
        assert getattr(lib, name) is not None
    for name in ("SketchGraph", "BuddyTwin", "run_buddy"):
        assert callable(getattr(s3grl_amd, name)) and callable(getattr(S, name))
    for method in ("ball_sizes", "features", "intersections", "raw", "close"):
        assert callable(getattr(S.SketchGraph, method))
    m, C, LC = S.hll_constants(8)
    rm, _, rC, rLC = R.constants(8)
    assert (m, C) == (rm, rC) and np.array_equal(LC, rLC)
    # through the C ABI: refusals that need no context and no GPU
    null = None
    assert lib.s3grl_sketch_build(null, 3, null, null, 0, 2, 128, 8, 0, null, null) != 0
    assert lib.s3grl_sketch_cardinality(null, 8, null, 1.0, null, 0, null) != 0
    assert lib.s3grl_sketch_pairs(null, 3, 2, 128, 8, null, null, null, 1.0, null, 0, null, null, null, null, null) != 0
