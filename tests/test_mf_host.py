"""Host checks of the MF baseline (no GPU): the fp64 restatement (tests/mf_reference.py) against torch autograd and
torch.optim.Adam; its fp32 sigmoid at saturated outputs; the lane layouts the GPU shape list reaches; how far outside
the GPU test's bounds each plausible kernel fault lands; every argument check; the ABI."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import mf_checks as K
import mf_reference as R

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def mf():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd import mf as module

    return module


# ---- the restatement against torch ---------------------------------------------------------------------------------
class TorchPredictor(torch.nn.Module):
    """The reference's structure written afresh: Linear, relu, dropout (as an explicit mask) per hidden layer."""

    def __init__(self, layers):
        super().__init__()
        self.lins = torch.nn.ModuleList()
        for W, b in layers:
            lin = torch.nn.Linear(W.shape[1], W.shape[0]).double()
            with torch.no_grad():
                lin.weight.copy_(torch.as_tensor(W))
                lin.bias.copy_(torch.as_tensor(b))
            self.lins.append(lin)

    def forward(self, xi, xj, masks, p):
        h = xi * xj
        for l, lin in enumerate(self.lins[:-1]):
            h = torch.relu(lin(h))
            if masks is not None:
                h = h * torch.as_tensor(masks[:, l, :], dtype=h.dtype) / (1 - p)
        return torch.sigmoid(self.lins[-1](h))[:, 0]


def torch_loss(emb, pred, pos, neg, masks, p):
    B = len(pos)
    pos, neg = torch.as_tensor(pos), torch.as_tensor(neg)
    sp = pred(emb[pos[:, 0]], emb[pos[:, 1]], None if masks is None else masks[:B], p)
    sn = pred(emb[neg[:, 0]], emb[neg[:, 1]], None if masks is None else masks[B:], p)
    return -torch.log(sp + 1e-15).mean() + -torch.log(1 - sn + 1e-15).mean()


@pytest.mark.parametrize("H,L,B,p", [(8, 3, 6, 0.5), (5, 2, 4, 0.0), (4, 4, 9, 0.25)])
def test_restatement_matches_torch_autograd_and_adam(H, L, B, p):
    rng = np.random.default_rng(3)
    n = 20
    x0, layers0 = K.init_params(n, H, L, seed=5)
    st = R.new_state(x0, layers0)
    emb = torch.nn.Parameter(torch.as_tensor(x0, dtype=torch.float64))
    pred = TorchPredictor([(W.astype(np.float64), b.astype(np.float64)) for W, b in layers0])
    opt = torch.optim.Adam([emb] + list(pred.parameters()), lr=0.01)
    for step in range(3):
        pos, neg = K.hub_pairs(B, rng, n)                      # duplicates, a self-pair, node n - 1 untouched
        masks = K.random_masks(B, L, H, p, rng) if p else None
        opt.zero_grad()
        loss = torch_loss(emb, pred, pos, neg, masks, p)
        loss.backward()
        opt.step()
        st, ref_loss = R.step(st, pos, neg, masks, p, 0.01)
        assert abs(ref_loss - float(loss.detach())) <= 1e-12 * abs(ref_loss)
        np.testing.assert_allclose(st["x"], emb.detach().numpy(), rtol=1e-9, atol=1e-12)
        state = opt.state[emb]
        np.testing.assert_allclose(st["xm"], state["exp_avg"].numpy(), rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(st["xv"], state["exp_avg_sq"].numpy(), rtol=1e-9, atol=1e-18)
        for (W, b), lin, (mW, mb), (vW, vb) in zip(st["layers"], pred.lins, st["lm"], st["lv"]):
            np.testing.assert_allclose(W, lin.weight.detach().numpy(), rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(b, lin.bias.detach().numpy(), rtol=1e-9, atol=1e-12)
            np.testing.assert_allclose(mW, opt.state[lin.weight]["exp_avg"].numpy(), rtol=1e-9, atol=1e-15)
            np.testing.assert_allclose(vb, opt.state[lin.bias]["exp_avg_sq"].numpy(), rtol=1e-9, atol=1e-18)
    # dense Adam: the row no pair ever touched has not moved, one touched only earlier keeps moving
    assert np.array_equal(st["x"][n - 1], x0[n - 1].astype(np.float64)) and not st["xm"][n - 1].any()


def test_fp32_sigmoid_at_saturated_outputs():
    x, layers = K.saturated_params()
    st = R.new_state(x, layers)
    loss, (ga, gb), glayers, aux = R.loss_and_grads(st["x"], st["layers"], K.SATURATED_POS, K.SATURATED_NEG, None, 0.0,
                                                    fp32_sigmoid=True)
    np.testing.assert_allclose(aux["out"], [18, -100, -18, 0, 18, -100, -18, 18])
    s32 = R.sigmoid(aux["out"], fp32=True)
    ts = torch.sigmoid(torch.as_tensor(aux["out"], dtype=torch.float32)).double().numpy()
    np.testing.assert_allclose(s32, ts, rtol=3e-7, atol=1e-37)
    assert s32[0] == 1.0 and s32[1] == 0.0                       # past 16.6 and at -100
    assert np.isfinite(loss) and all(np.isfinite(g).all() for pair in glayers for g in pair)
    g = aux["g"]
    assert g[4] == 0.0 and g[7] == 0.0                           # 1 - s is exactly 0: EPS-form derivative 0
    assert g[1] == 0.0                                           # s is exactly 0
    # in fp64 the same negatives still have a derivative of about s / B
    g64 = R.loss_and_grads(st["x"], st["layers"], K.SATURATED_POS, K.SATURATED_NEG, None, 0.0)[3]["g"]
    assert g64[4] > 0.2
    # torch in fp32 takes the same values
    emb = torch.nn.Parameter(torch.as_tensor(x))
    pred = TorchPredictor(layers).float()
    tl = torch_loss(emb, pred, K.SATURATED_POS, K.SATURATED_NEG, None, 0.0)
    tl.backward()
    assert abs(float(tl.detach()) - loss) <= 1e-5 * loss
    gx = R.table_grad(len(x), aux["pairs"], ga, gb)
    np.testing.assert_allclose(gx, emb.grad.double().numpy(), rtol=1e-4, atol=1e-6)


# ---- layouts -------------------------------------------------------------------------------------------------------
def test_shape_list_reaches_every_layout(mf):
    seen = set()
    for shape in K.SHAPES:
        H, L, B = K.resolve(shape, mf.layout)
        lay = mf.layout(H, L, B)
        assert lay["tiles"] == -(-2 * B // lay["pairs_per_tile"])
        assert lay["channels_per_lane"] * lay["lanes_per_pair"] >= H
        seen.add((lay["channels_per_lane"], lay["lanes_per_pair"], lay["pairs_per_tile"]))
    every = {tuple(mf.layout(H, 2, 1)[k] for k in ("channels_per_lane", "lanes_per_pair", "pairs_per_tile"))
             for H in range(1, 129)}
    assert every == K.LAYOUTS == seen
    Hs, Ls, Bs = ({K.resolve(s, mf.layout)[i] for s in K.SHAPES} for i in range(3))
    assert {1, 3, 32, 33, 128} <= Hs and Ls == {2, 3, 4} and {1, 5, 32, 33, 17, 1024} <= Bs
    assert max(K.resolve(s, mf.layout)[2] * 2 // mf.layout(s[0], s[1], 1)["pairs_per_tile"] for s in K.SHAPES) > 1


# ---- faults --------------------------------------------------------------------------------------------------------
def test_every_fault_lands_far_outside_the_bounds(mf):
    """Each fault's worst |faulty - restatement| / bound over the state, after one clean step so that moments are
    non-zero (shape H = 32, 3 layers, B = 33: five tiles, the last one short).  Measured factors: duplicate_dropped
    3.4e3, self_pair_b_dropped 4.3e3, no_decay_of_untouched_rows 7.5e5, last_channel_missed 1.7e4,
    last_tile_partial_dropped 4.8e5, one_mask_for_both 2.3e28 (a moment whose bound is its 1e-36 floor)."""
    H, L, B, p, lr = 32, 3, 33, 0.5, 0.01
    tile = mf.layout(H, L, B)["pairs_per_tile"]
    rng = np.random.default_rng(11)
    x0, layers0 = K.init_params(K.HUB_N, H, L, seed=2)
    st = R.new_state(x0, layers0)
    pos, neg = K.hub_pairs(B, rng)
    st, _ = R.step(st, pos, neg, K.random_masks(B, L, H, p, rng), p, lr, fp32_sigmoid=True)
    pos, neg = K.hub_pairs(B, rng)
    masks = K.random_masks(B, L, H, p, rng)
    clean, _, bounds = K.step_bounds(st, pos, neg, masks, p, lr)
    factors = {}
    for fault in K.FAULTS:
        bad = K.faulty_step(st, pos, neg, masks, p, lr, fault, tile)
        factors[fault] = max(K.worst_ratio(bad, clean, bounds).values())
    print({k: f"{v:.1e}" for k, v in factors.items()})
    assert all(v > 100 for v in factors.values()), factors
    assert max(K.worst_ratio(clean, clean, bounds).values()) == 0.0


# ---- arguments -----------------------------------------------------------------------------------------------------
def test_argument_checks(mf):
    T = mf.MFTrainer
    for bad in (dict(hidden=129), dict(num_layers=1), dict(num_layers=5)):
        kw = dict(num_nodes=10, hidden=8, num_layers=3, dropout=0.5, lr=0.01)
        kw.update(bad)
        with pytest.raises(NotImplementedError, match=r"128|2\.\.4"):
            T(**kw)
    with pytest.raises(NotImplementedError, match="1024"):
        mf.layout(8, 3, 1025)
    for bad in (dict(num_nodes=0), dict(hidden=0), dict(dropout=1.0), dict(dropout=-0.1), dict(lr=0.0),
                dict(lr=float("nan"))):
        kw = dict(num_nodes=10, hidden=8, num_layers=3, dropout=0.5, lr=0.01)
        kw.update(bad)
        with pytest.raises(ValueError):
            T(**kw)
    x, layers = K.init_params(10, 8, 3, 0)
    with pytest.raises(ValueError, match="init table"):
        T(11, 8, 3, 0.5, 0.01, init=(x, layers))
    with pytest.raises(ValueError, match="init needs"):
        T(10, 8, 3, 0.5, 0.01, init=(x, layers[:2]))
    with pytest.raises(ValueError, match="init layer 2"):
        T(10, 8, 3, 0.5, 0.01, init=(x, layers[:2] + [layers[0]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T(10, 8, 3, 0.5, 0.01, device="cpu")
    for pairs, msg in ((np.zeros((3, 3), dtype=np.int64), r"\[P, 2\]"), (np.zeros((3, 2)), "integer"),
                       (np.array([[0, 10]]), "outside"), (np.array([[-1, 0]]), "outside"),
                       (np.zeros((0, 2), dtype=np.int64), "empty")):
        with pytest.raises(ValueError, match=msg):
            mf._pairs(pairs, 10, "pairs")
    split = {s: {"edge": np.array([[0, 1], [1, 2]]), "edge_neg": np.array([[0, 2], [3, 4]])}
             for s in ("train", "valid", "test")}
    data, args = SimpleNamespace(num_nodes=5), SimpleNamespace(res_dir="")
    call = dict(data=data, split_edge=split, device=None, log_steps=1, num_layers=3, hidden_channels=8, dropout=0.5,
                batch_size=2, lr=0.01, epochs=2, eval_steps=1, runs=1, seed=1, args=args)
    for bad, exc in ((dict(epochs=-1), ValueError), (dict(eval_steps=0), ValueError), (dict(runs=0), ValueError),
                     (dict(lr=0.0), ValueError), (dict(batch_size=0), ValueError),
                     (dict(batch_size=2000), NotImplementedError), (dict(hidden_channels=200), NotImplementedError),
                     (dict(data=SimpleNamespace(num_nodes=4)), ValueError),
                     (dict(split_edge={"train": split["train"]}), ValueError)):
        with pytest.raises(exc):
            mf.train_mf(**{**call, **bad})


# ---- must fail without the feature ---------------------------------------------------------------------------------
def test_mf_is_part_of_the_abi(mf):
    from s3grl_amd import _native

    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_mf_[a-z_]+)\s*\(", header))
    assert declared == {"s3grl_mf_layout", "s3grl_mf_create", "s3grl_mf_epoch", "s3grl_mf_step_pairs",
                        "s3grl_mf_export_draws", "s3grl_mf_score", "s3grl_mf_state", "s3grl_mf_destroy"}
    assert declared <= set(_native.SYMBOLS)
    for name in declared:
        assert getattr(_native.lib(), name) is not None
    import s3grl_amd

    assert callable(s3grl_amd.run_mf) and callable(s3grl_amd.train_mf) and callable(s3grl_amd.MFTrainer)
    assert "s3grl_mf.hip" in __import__("__graft_entry__").SOURCES
