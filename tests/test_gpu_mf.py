"""The MF baseline on the MI355X (s3grl_amd.mf, csrc/s3grl_mf.hip): dense Adam on rows no step touches, the dropout
masks and negative pairs the engine draws, saturated outputs, determinism and the replay of an epoch through the
teacher-forcing hook, `score`, and the Table 2 row on USAir end to end."""
import numpy as np
import pytest
import torch

import mf_checks as K
import mf_reference as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def usair():
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    return W.edge_split(n, e, seed=0)


def _trainer(H=32, L=3, p=0.5, n=K.HUB_N, seed=0, init_seed=1, lr=0.01):
    from s3grl_amd.mf import MFTrainer

    x0, layers0 = K.init_params(n, H, L, seed=init_seed)
    return MFTrainer(n, H, L, p, lr, seed=seed, init=(x0, layers0)), x0


def test_dense_adam_moves_rows_the_step_does_not_touch():
    mf, x0 = _trainer(H=13, L=3, p=0.0)
    rng = np.random.default_rng(4)
    set1, set2 = np.arange(0, 20), np.arange(20, 40)             # nodes 40.. are in no step
    worst = {}
    pairs1 = rng.choice(set1, (12, 2))
    K.step_check(mf, pairs1[:6], pairs1[6:], None, 0.0, worst, "step 1")
    after1 = K.state_of(mf)
    pairs2 = rng.choice(set2, (12, 2))
    K.step_check(mf, pairs2[:6], pairs2[6:], None, 0.0, worst, "step 2")      # inside the restatement's bounds
    after2 = K.state_of(mf)
    touched1 = np.unique(pairs1)
    assert not np.intersect1d(touched1, np.unique(pairs2)).size
    # set 1's rows: no gradient in step 2, yet the moments decayed and the weights moved
    np.testing.assert_allclose(after2["xm"][touched1], 0.9 * after1["xm"][touched1], rtol=1e-6)
    np.testing.assert_allclose(after2["xv"][touched1], 0.999 * after1["xv"][touched1], rtol=1e-6)
    assert (after2["x"][touched1] != after1["x"][touched1]).all()
    never = np.arange(40, K.HUB_N)
    assert np.array_equal(after2["x"][never], x0[never].astype(np.float64))
    assert not after2["xm"][never].any() and not after2["xv"][never].any()
    mf.close()


def test_masks_and_negatives_the_engine_draws():
    from s3grl_amd.mf import MFTrainer

    n, H, L, B = 13, 32, 3, 64
    keep, neg_count = [], np.zeros(n)
    m0 = MFTrainer(n, H, L, 0.0, 0.01, seed=5)
    assert bool(m0.draws(0, 0, 1000, B)[2].all())                              # p = 0: all kept
    m0.close()
    mf = MFTrainer(n, H, L, 0.5, 0.01, seed=5)
    seen = set()
    for step in range(4):
        idx, neg, masks = mf.draws(1, step, 1000, B)
        assert idx.shape == (B,) and neg.shape == (B, 2) and masks.shape == (2 * B, L - 1, H)
        m = masks.cpu().numpy()
        assert set(np.unique(m)) <= {0, 1}
        assert not np.array_equal(m[:B], m[B:])                                  # positives and negatives differ
        keep.append(m.reshape(-1))
        neg_count += np.bincount(neg.cpu().numpy().reshape(-1), minlength=n)
        seen.update(idx.cpu().tolist())
        assert int(neg.min()) >= 0 and int(neg.max()) < n
    assert len(seen) == 4 * B and max(seen) < 1000                              # distinct positions of one permutation
    keep = np.concatenate(keep)
    assert keep.size >= 10000
    # chi-square at 1e-4: 1 degree of freedom -> 15.14; 12 degrees -> 39.13
    k1 = keep.sum()
    chi_keep = (k1 - keep.size / 2) ** 2 / (keep.size / 4)
    assert chi_keep < 15.14, (k1, keep.size)
    exp = neg_count.sum() / n
    chi_neg = ((neg_count - exp) ** 2 / exp).sum()
    assert chi_neg < 39.13, neg_count
    mf.close()


def test_saturated_outputs_stay_finite_and_inside_the_bounds():
    from s3grl_amd.mf import MFTrainer

    x, layers = K.saturated_params()
    mf = MFTrainer(len(x), 4, 2, 0.0, 0.01, seed=0, init=(x, layers))
    out = R.forward(x.astype(np.float64), [(W.astype(np.float64), b.astype(np.float64)) for W, b in layers],
                    np.concatenate([K.SATURATED_POS, K.SATURATED_NEG]))[2]
    assert out.max() >= 17 and out.min() == -100 and not ((out > 16.3) & (out < 17)).any()
    worst = {}
    for step in range(3):
        loss, ref = K.step_check(mf, K.SATURATED_POS, K.SATURATED_NEG, None, 0.0, worst, f"saturated step {step}")
    got = K.state_of(mf)
    assert all(np.isfinite(got[k]).all() for k in ("x", "xm", "xv"))
    assert all(np.isfinite(t).all() for k in ("layers", "lm", "lv") for pair in got[k] for t in pair)
    mf.close()


def test_one_seed_is_bit_identical_and_an_epoch_replays_through_the_hook():
    from s3grl_amd.mf import MFTrainer

    n, H, L, p, B = 50, 32, 3, 0.5, 32
    rng = np.random.default_rng(8)
    train = rng.integers(0, n, (B * 3 + 7, 2))                                  # the last batch is short: 7 pairs
    a, b, twin = (MFTrainer(n, H, L, p, 0.01, seed=21) for _ in range(3))
    la = [a.fit_epoch(train, B) for _ in range(2)]
    lb = [b.fit_epoch(train, B) for _ in range(2)]
    assert la == lb and K.same_state(a, b)
    other = MFTrainer(n, H, L, p, 0.01, seed=22)
    other.fit_epoch(train, B)
    assert not torch.equal(other.state()["weight"], a.state()["weight"])
    tt = torch.as_tensor(train)
    for epoch in range(2):
        total = 0.0
        for step in range(4):
            idx, neg, masks = twin.draws(epoch, step, len(train), B)
            assert len(idx) == (7 if step == 3 else B)
            total += twin.step(tt[idx.cpu()], neg, masks) * len(idx)
        assert abs(total / len(train) - la[epoch]) <= 1e-6 * abs(la[epoch])
    assert K.same_state(a, twin)
    assert a.state()["step"] == 8
    for t in (a, b, twin, other):
        t.close()


def test_score_is_the_eval_forward():
    mf, _ = _trainer(H=33, L=4, p=0.5)
    rng = np.random.default_rng(2)
    pos, neg = K.hub_pairs(8, rng)
    mf.step(pos, neg)
    pairs = rng.integers(0, K.HUB_N, (41, 2))
    pairs[5] = pairs[4]
    pairs[9] = (3, 3)
    got = mf.score(pairs).cpu().double().numpy()
    ref = R.score(K.state_of(mf), pairs, fp32_sigmoid=True)
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=1e-7)
    assert got[5] == got[4]
    empty = mf.score(np.zeros((0, 2), dtype=np.int64))
    assert empty.shape == (0,) and empty.dtype == torch.float32
    with pytest.raises(ValueError, match="outside"):
        mf.score(np.array([[0, K.HUB_N]]))
    mf.close()


# The eager-torch loop of the reference's structure (tools/mf_probe.py torch_mf) on 16 CPU threads, USAir split of seed
# 0, seeds 1, 2, 3: test AUC TORCH_AUC (the engine: 0.8942, 0.9168, 0.8985).  The engine's streams differ, so its floor
# is that minimum minus the loop's own max - min spread, the margin at least 0.01.
TORCH_AUC = (0.8979, 0.9061, 0.8903)
FLOOR = min(TORCH_AUC) - max(max(TORCH_AUC) - min(TORCH_AUC), 0.01)      # 0.8745


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_table2_usair(usair, seed):
    from s3grl_amd import mf as M

    res = M.run_mf(usair, seed=seed, device=DEV)
    print("MF USAir seed", seed, res)
    assert 0 <= res["AP"][1] <= 1
    assert res["AUC"][1] >= FLOOR


def test_train_mf_with_the_reference_signature(usair, tmp_path):
    from types import SimpleNamespace

    from s3grl_amd import mf as M

    args = SimpleNamespace(res_dir=str(tmp_path), epochs=3)
    data = SimpleNamespace(num_nodes=usair.num_nodes)
    auc = M.train_mf(data, usair.split_edge(), DEV, 1, 3, 32, 0.5, 32, 0.01, 3, 1, 2, 1, args)
    assert 0 < auc <= 100
    log = (tmp_path / "log.txt").read_text()
    assert log.count("Run: 01, Epoch: 03") == 2 and log.count("Run: 02") == 6       # AUC and AP, every epoch
    quiet = SimpleNamespace(res_dir="", epochs=3)
    assert M.train_mf(data, usair.split_edge(), DEV, 1, 3, 32, 0.5, 32, 0.01, 3, 1, 1, 1, quiet) == auc
