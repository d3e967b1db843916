"""node2vec's step kernels (csrc/s3grl_node2vec.hip) where tests/test_gpu_node2vec.py does not reach: every (VEC, LPD)
lane layout of dots_kernel / row_grad_kernel / adam_kernel from a caller's `init=` table, sigmoid saturation on both
sides, rows a step does not touch (bit for bit), the smallest windows and batches, the distribution of the negative
draws and of duplicated arcs, and buffers that grow during an object's life.

The reference is the fp64 restatement (tests/node2vec_reference.py, sigmoid in fp32 as the reference trains) and the
bound is `tolerances` of tests/node2vec_checks.py, unchanged: 1e-5 · Σ|g · h| per gradient element, carried through
SparseAdam, for rows of at most 4 400 terms.  tests/test_node2vec_host.py shows on the CPU that a dropped term, a
dropped slice or a missed channel lands hundreds of times outside it in exp_avg and exp_avg_sq (not in the weight at
the first step), so every case asserts all three tensors and takes steps from non-zero moments.  Every parity test
prints its worst error / bound; above 1 is a failure."""
import numpy as np
import pytest
import torch

from node2vec_checks import (DIMS, HUB_BS, HUB_CFG, check_windows, dots_of, hub_graph, init_table, lanes_rule, parity,
                             row_uses, same_state, step_check, walks_of)

pytestmark = pytest.mark.gpu


def _dot_range(limit=12.0):
    def check(h, pos, neg):
        worst = max(float(np.abs(dots_of(h, w)).max()) for w in (pos, neg))
        assert worst < limit, worst          # no sigmoid near saturation: every gradient term is alive
    return check


def _replay(n2v, epoch, bs):
    return [n2v.step(*n2v.windows(epoch, s, bs)) for s in range(n2v.steps_per_epoch(bs))]


# ---- 1. every lane layout ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", sorted(DIMS))
def test_step_kernels_at_every_lane_layout(D):
    """Three teacher-forced steps on the hub graph (node 0 collects a few hundred terms a step, so each of
    row_grad_kernel's 64 / LPD slices loops; node 69 has no edges), then an epoch drawn by the engine against the
    same epoch replayed through the step hook on a twin, bit for bit."""
    from s3grl_amd.node2vec import Node2Vec

    assert lanes_rule(D) == DIMS[D]
    ei, n = hub_graph()
    assert not np.isin(ei, n - 1).any() and not np.isin(ei[0], n - 2).any()
    init = init_table(n, D, seed=D)
    a, b = (Node2Vec(ei, n, D, seed=5, init=init, **HUB_CFG) for _ in range(2))
    assert torch.equal(a.embedding().cpu(), init) and a.state()["step"] == 0      # the table as given, bit for bit
    assert not a.state()["exp_avg"].any() and not a.state()["exp_avg_sq"].any()
    uses = [row_uses(*(x.cpu().numpy() for x in a.windows(0, s, HUB_BS)), 0) for s in range(3)]
    assert all(64 < u <= 4400 for u in uses), uses
    worst = parity(a, 3, bs=HUB_BS, before_step=_dot_range())
    print(f"[n2v shapes] D={D} {lanes_rule(D)} hub terms {uses}: worst error / bound h {worst[0]:.3g} m {worst[1]:.3g} "
          f"v {worst[2]:.3g}, loss rel {worst[3]:.3g}")
    for s in range(3):
        b.step(*b.windows(0, s, HUB_BS))
    assert same_state(a, b)
    la = a.fit(1, batch_size=HUB_BS)
    lb = _replay(b, 0, HUB_BS)
    assert same_state(a, b) and a.state()["step"] == 3 + a.steps_per_epoch(HUB_BS)
    np.testing.assert_allclose(la, [sum(lb)], rtol=1e-6)   # per-step losses are identical; the host sums in another order
    assert torch.isfinite(a.embedding()).all()


# ---- 3. saturation -------------------------------------------------------------------------------------------------
def _saturation_case(D):
    """40 rows along one unit direction e plus small noise.  Rows 0, 1: 4.5 e and 4.6 e (their dot is 20.7: as a
    negative dot, fp32 1 - s is 0).  Rows 2, 3: 10 e and -10 e (-100: as a positive dot, expf overflows and s is 0).
    Rows 4..39: N(0, 1) · 0.8 / sqrt(D), dots of a few tenths among themselves.  Windows of 3 nodes."""
    rng = np.random.default_rng(100 + D)
    e = rng.standard_normal(D)
    e /= np.linalg.norm(e)
    h = rng.standard_normal((40, D)) * 0.8 / np.sqrt(D)
    for row, a in ((0, 4.5), (1, 4.6), (2, 10.0), (3, -10.0)):
        h[row] = a * e + 0.01 * h[row]
    small = np.arange(4, 40)
    pos = np.concatenate([
        [[2, 3, 3], [3, 2, 2], [2, 3, 7]],                    # below -90 (and one dot with a small row)
        [[5, 5, 6], [9, 8, 9]],                               # self-dots: the row's gradient is 2 · g · h
        rng.choice(small, (40, 3)),
    ])
    neg = np.concatenate([
        [[0, 1, 1], [1, 0, 12], [0, 0, 1], [2, 0, 1]],        # past 18: 20.7, 20.25 (a saturated self-dot), 45, 46
        [[11, 11, 4]],
        rng.choice(small, (40, 3)),
    ])
    return torch.as_tensor(h, dtype=torch.float32), pos, neg


@pytest.mark.parametrize("D", [3, 20])
def test_saturated_dots_on_both_sides(D):
    from s3grl_amd.node2vec import Node2Vec

    init, pos, neg = _saturation_case(D)
    n2v = Node2Vec(np.zeros((2, 0), dtype=np.int64), 40, D, context_size=3, walk_length=3, seed=0, init=init)

    def groups(h, pos, neg):
        op, on = dots_of(h, pos), dots_of(h, neg)
        assert not ((on >= 15) & (on <= 18.5)).any()          # the jump of a negative dot's gradient (out ~ 16.6)
        counts = (int((on > 18).sum()), int((op < -90).sum()), int((np.abs(op) < 5).sum()),
                  int((np.abs(on) < 5).sum()))
        assert min(counts) > 0, counts
        mid = np.concatenate([op[np.abs(op) < 5], on[np.abs(on) < 5]])
        assert (mid > 0).any() and (mid < 0).any()
        selfs = [w[:, :1] == w[:, 1:] for w in (pos, neg)]
        assert (np.abs(op[selfs[0]]) < 5).sum() >= 2 and (np.abs(on[selfs[1]]) < 5).sum() >= 1
        assert (on[selfs[1]] > 18).any()

    worst = [0.0] * 4
    for t in range(2):
        loss, ref_loss = step_check(n2v, pos, neg, 0.01, worst, f"step {t}", saturated_past=18.5, before_step=groups)
        assert np.isfinite(loss) and np.isfinite(ref_loss)
        st = n2v.state()
        assert all(torch.isfinite(st[k]).all() for k in ("weight", "exp_avg", "exp_avg_sq"))
    # rows 2 and 3 meet saturated dots only, apart from row 2's one dot with row 7: row 3's gradient is exactly 0
    assert not st["exp_avg"][3].any() and not st["exp_avg_sq"][3].any() and torch.equal(st["weight"][3].cpu(), init[3])
    print(f"[n2v shapes] saturation D={D}: worst error / bound h {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g}, "
          f"loss rel {worst[3]:.3g}")


# ---- 4. untouched rows, bit for bit --------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 20, 260])
def test_rows_a_step_does_not_touch_keep_their_bits(D):
    from s3grl_amd.node2vec import Node2Vec

    n = 60
    A, B, rest = slice(0, 20), slice(20, 40), slice(40, 60)
    rng = np.random.default_rng(D)
    init = init_table(n, D, seed=40 + D)
    n2v = Node2Vec(np.zeros((2, 0), dtype=np.int64), n, D, context_size=3, walk_length=3, seed=0, init=init)
    wins = {k: (rng.integers(s.start, s.stop, (50, 3)), rng.integers(s.start, s.stop, (70, 3)))
            for k, s in (("A", A), ("B", B))}
    for k, s in (("A", A), ("B", B)):                         # each set is used in full and nothing else is
        assert np.array_equal(np.unique(np.concatenate(wins[k])), np.arange(s.start, s.stop))
    worst = [0.0] * 4
    keys = ("weight", "exp_avg", "exp_avg_sq")
    step_check(n2v, *wins["A"], 0.01, worst, "step A", before_step=_dot_range())
    s1 = n2v.state()
    assert all(s1[k][A].abs().sum() > 0 for k in keys[1:])
    step_check(n2v, *wins["B"], 0.01, worst, "step B", before_step=_dot_range())   # bias correction of step 2
    s2 = n2v.state()
    assert s2["step"] == 2
    for k in keys:
        assert torch.equal(s2[k][A], s1[k][A]) and torch.equal(s2[k][rest], s1[k][rest]), k
        assert not torch.equal(s2[k][B], s1[k][B]), k
    assert torch.equal(s2["weight"][rest].cpu(), init[rest])
    assert not s2["exp_avg"][rest].any() and not s2["exp_avg_sq"][rest].any()
    step_check(n2v, *wins["A"], 0.01, worst, "step A again", before_step=_dot_range())   # a stamp two steps old
    s3 = n2v.state()
    for k in keys:
        assert torch.equal(s3[k][B], s2[k][B]) and torch.equal(s3[k][rest], s1[k][rest]), k
    print(f"[n2v shapes] untouched rows D={D}: worst error / bound h {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g}")


# ---- 5. window edges -----------------------------------------------------------------------------------------------
EDGES = {
    "context_size=2": dict(n=50, bs=16, cfg=dict(walk_length=5, context_size=2, walks_per_node=2)),
    "walk_length=context_size": dict(n=50, bs=16, cfg=dict(walk_length=4, context_size=4, walks_per_node=2)),
    "walks_per_node=1": dict(n=50, bs=16, cfg=dict(walk_length=6, context_size=3, walks_per_node=1)),
    "num_negative_samples=3": dict(n=50, bs=16, cfg=dict(walk_length=6, context_size=3, walks_per_node=2,
                                                         num_negative_samples=3)),
    "batch_size=1": dict(n=50, bs=1, cfg=dict(walk_length=6, context_size=3, walks_per_node=2)),
    "batch_size>N": dict(n=50, bs=64, cfg=dict(walk_length=6, context_size=3, walks_per_node=2)),
    "all at once": dict(n=41, bs=1, cfg=dict(walk_length=2, context_size=2, walks_per_node=1, num_negative_samples=3)),
    "N=1": dict(n=1, bs=16, cfg=dict(walk_length=6, context_size=3, walks_per_node=2)),
}


@pytest.mark.parametrize("D", [8, 5])
@pytest.mark.parametrize("name", list(EDGES))
def test_window_edges(name, D):
    from s3grl_amd.node2vec import Node2Vec

    n, bs, cfg = (EDGES[name][k] for k in ("n", "bs", "cfg"))
    if n > 1:
        ei, _ = hub_graph(n)
    else:
        ei = np.zeros((2, 0), dtype=np.int64)
    n2v = Node2Vec(ei, n, D, seed=2, init=init_table(n, D, seed=n + D, c=1.0), **cfg)
    for epoch in (0, 3):
        check_windows(n2v, ei, n, epoch, bs=bs)
    if n == 1:
        pos, neg = n2v.windows(0, 0, bs)
        assert not pos.any() and not neg.any() and pos.shape == (5 * 2, 3)   # every window is the node itself
    worst = parity(n2v, 1 if n == 1 else 2, bs=bs, before_step=_dot_range())
    st = n2v.state()
    assert all(torch.isfinite(st[k]).all() for k in ("weight", "exp_avg", "exp_avg_sq"))
    print(f"[n2v shapes] {name} D={D}: worst error / bound h {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g}, "
          f"loss rel {worst[3]:.3g}")


# ---- 6. distributions ----------------------------------------------------------------------------------------------
def test_negative_draws_are_uniform_over_the_nodes():
    """Every node of a negative row after its start is one draw from [0, N).  N = 13, 5 epochs of one step with
    10 rows of 20 draws per node: 13 000 draws, chi-square with 12 degrees of freedom, P(chi2 > 39.2) < 1e-4; the
    draws of one walk position alone (650 each) against the same threshold."""
    from s3grl_amd.node2vec import Node2Vec

    n, L, C = 13, 20, 10
    ring = np.array([np.arange(n), (np.arange(n) + 1) % n])
    n2v = Node2Vec(ring, n, 4, walk_length=L, context_size=C, walks_per_node=10, seed=17)
    draws = []
    for e in range(5):
        _, neg = n2v.windows(e, 0, n)
        rows = walks_of(neg.cpu().numpy(), n * 10, C, L + 2 - C)
        assert rows.shape == (n * 10, L + 1)
        draws.append(rows[:, 1:])
    draws = np.concatenate(draws)

    def chi2(x):
        obs = np.bincount(x.reshape(-1), minlength=n)
        exp = obs.sum() / n
        return float(((obs - exp) ** 2 / exp).sum()), obs

    total, obs = chi2(draws)
    print(f"[n2v shapes] negative draws: chi2 {total:.3g} over {obs.sum()} draws, 12 dof")
    assert obs.sum() == 13_000 and total < 39.2, (obs, total)
    per_position = [chi2(draws[:, s])[0] for s in range(L)]
    assert max(per_position) < 39.2, per_position
    # the draws do not follow the start node: over the 50 rows of one start, the first draw is spread too
    first_by_start = [len(np.unique(draws[np.arange(len(draws)) % n == b, 0])) for b in range(n)]
    assert min(first_by_start) >= 8, first_by_start


def test_a_duplicated_arc_is_drawn_twice_as_often():
    """16 sources 3i with arcs to 3i + 1 twice and to 3i + 2 once (duplicates count, as in PyG's CSR).  11 200 first
    steps: two cells, expected 2/3 and 1/3, chi-square with 1 degree of freedom, P(chi2 > 15.2) < 1e-4."""
    from s3grl_amd.node2vec import Node2Vec

    k = 16
    s = 3 * np.arange(k)
    ei = np.stack([np.concatenate([s, s, s, s + 1, s + 2]), np.concatenate([s + 1, s + 2, s + 1, s, s])])
    n2v = Node2Vec(ei, 3 * k, 4, walk_length=2, context_size=2, walks_per_node=100, seed=23)
    to_u = to_v = 0
    for e in range(7):
        pos, _ = n2v.windows(e, 0, 3 * k)
        pos = pos.cpu().numpy()[:3 * k * 100]                  # window 0 of every walk: (start, first step)
        src = pos[pos[:, 0] % 3 == 0]
        assert len(src) == k * 100
        to_u += int((src[:, 1] == src[:, 0] + 1).sum())
        to_v += int((src[:, 1] == src[:, 0] + 2).sum())
    total = to_u + to_v
    assert total == 11_200
    chi2 = (to_u - total * 2 / 3) ** 2 / (total * 2 / 3) + (to_v - total / 3) ** 2 / (total / 3)
    print(f"[n2v shapes] duplicated arc: {to_u} to u, {to_v} to v, chi2 {chi2:.3g}, 1 dof")
    assert chi2 < 15.2, (to_u, to_v, chi2)


# ---- 7. growth during an object's life -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 65])
def test_buffers_grow_during_an_objects_life(D):
    """fit with batch size 8, then 64 (ensure_windows and the sort workspace grow between two epochs), against a twin
    that replays both epochs through the step hook; then a step with more windows than either epoch used."""
    from s3grl_amd.node2vec import Node2Vec

    ei, n = hub_graph()
    init = init_table(n, D, seed=3)
    a, b = (Node2Vec(ei, n, D, seed=8, init=init, **HUB_CFG) for _ in range(2))
    la = a.fit(1, batch_size=8) + a.fit(1, batch_size=64)
    lb = [sum(_replay(b, 0, 8)), sum(_replay(b, 1, 64))]
    assert same_state(a, b) and a.state()["step"] == 9 + 2
    np.testing.assert_allclose(la, lb, rtol=1e-6)
    epoch_windows = 5 * 64 * 2 * 2                             # W · B · walks_per_node · (1 + negatives)
    rng = np.random.default_rng(D)
    pos, neg = rng.integers(0, n, (1100, 3)), rng.integers(0, n, (900, 3))
    assert len(pos) + len(neg) > epoch_windows
    assert max(row_uses(pos, neg, u) for u in range(n)) <= 4400
    worst = [0.0] * 4
    step_check(a, pos, neg, 0.01, worst, "grown step", before_step=_dot_range())
    b.step(pos, neg)
    assert same_state(a, b)
    la = a.fit(1, batch_size=8)                                # and back to small batches in the grown buffers
    assert not same_state(a, b) and np.isfinite(la).all()
    _replay(b, 2, 8)
    assert same_state(a, b)
    print(f"[n2v shapes] grown step D={D}: worst error / bound h {worst[0]:.3g} m {worst[1]:.3g} v {worst[2]:.3g}, "
          f"loss rel {worst[3]:.3g}")
