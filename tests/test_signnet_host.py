"""Host checks of the fused SIGNNet trainer (no GPU): the fp64 restatement (tests/signnet_reference.py) against torch
autograd and torch.optim.Adam on a module built like `SIGNNetTwin`; the layouts the GPU shape list reaches; the
conditions on the GPU test's inputs; how far outside the GPU test's bounds each plausible kernel fault lands; every
argument check; the ABI."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
from torch import nn

import signnet_checks as K
import signnet_reference as R

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def signnet():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd import signnet as module

    return module


# ---- the restatement against torch ---------------------------------------------------------------------------------
class TorchNet(nn.Module):
    """`SIGNNetTwin`'s two stacks in double precision; dropout as explicit masks, the pool by plain indexing."""

    def __init__(self, in_width, hidden, ch):
        super().__init__()
        self.operator_diff = nn.Sequential(nn.Linear(in_width, hidden), nn.ELU(), nn.BatchNorm1d(hidden)).double()
        self.link_pred_mlp = nn.Sequential(nn.Linear(hidden * ch, hidden), nn.ReLU(), nn.BatchNorm1d(hidden)).double()
        self.last = nn.Linear(hidden, 1).double()

    def forward(self, X, lptr, mask1, mask2, p, mode):
        h = self.operator_diff(X)
        if mask1 is not None:
            h = h * torch.as_tensor(mask1, dtype=h.dtype) / (1 - p)
        z = h[lptr[:-1]] * h[lptr[:-1] + 1]
        if mode:
            pooled = []
            for b in range(len(lptr) - 1):
                rest = h[lptr[b] + 2:lptr[b + 1]]
                if not len(rest):
                    pooled.append(torch.zeros_like(h[0]))
                else:
                    pooled.append(rest.mean(0) if mode == "mean" else rest.sum(0))
            z = torch.cat([z, torch.stack(pooled)], dim=1)
        d = self.link_pred_mlp(z)
        if mask2 is not None:
            d = d * torch.as_tensor(mask2, dtype=d.dtype) / (1 - p)
        return self.last(d).view(-1)


@pytest.mark.parametrize("mode,kind,p", [("", "two", 0.5), ("mean", "mixed", 0.5), ("sum", "mixed", 0.0)])
def test_restatement_matches_torch_autograd_and_adam(mode, kind, p):
    H, IW, B, lr = 6, 5, 7, 0.01
    case = K.Case(H, IW, B, p, mode, kind, seed=3, lr=lr)
    x, row_ptr, y = case.store
    st = case.state0()
    net = TorchNet(IW, H, case.ch)
    mods = (net.operator_diff[0], net.operator_diff[2], net.link_pred_mlp[0], net.link_pred_mlp[2], net.last)
    tensors = [t for m in mods for t in (m.weight, m.bias)]
    with torch.no_grad():
        for t, name in zip(tensors, R.NAMES):
            t.copy_(torch.as_tensor(st[name]))
    opt = torch.optim.Adam(tensors, lr=lr)
    net.train()
    for ids, m1, m2 in case.batches(3):
        ridx, lptr = R.batch_rows(row_ptr, ids)
        opt.zero_grad()
        out = net(torch.as_tensor(x[ridx], dtype=torch.float64), lptr, m1, m2, p, mode)
        loss = nn.functional.binary_cross_entropy_with_logits(out, torch.as_tensor(y[ids], dtype=torch.float64))
        loss.backward()
        opt.step()
        st, ref_loss, _, _ = R.step(st, x, row_ptr, y, ids, m1, m2, p, mode, lr)
        assert abs(ref_loss - float(loss.detach())) <= 1e-12 * abs(ref_loss)
        for t, name in zip(tensors, R.NAMES):
            np.testing.assert_allclose(st[name], t.detach().numpy(), rtol=1e-9, atol=1e-12, err_msg=name)
            np.testing.assert_allclose(st["m"][name], opt.state[t]["exp_avg"].numpy(), rtol=1e-8, atol=1e-15)
            np.testing.assert_allclose(st["v"][name], opt.state[t]["exp_avg_sq"].numpy(), rtol=1e-8, atol=1e-18)
        for bn, (rm, rv) in ((net.operator_diff[2], ("rm1", "rv1")), (net.link_pred_mlp[2], ("rm2", "rv2"))):
            np.testing.assert_allclose(st[rm], bn.running_mean.numpy(), rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(st[rv], bn.running_var.numpy(), rtol=1e-12, atol=1e-15)
            assert int(bn.num_batches_tracked) == st["nbt"]
    net.eval()
    ref = R.score(st, x, row_ptr, mode)
    with torch.no_grad():
        got = net(torch.as_tensor(x, dtype=torch.float64), row_ptr, None, None, 0.0, mode).numpy()
    np.testing.assert_allclose(ref, got, rtol=1e-10, atol=1e-12)


def test_fp32_restatement_is_close_and_depends_on_the_order():
    case = K.Case(32, 64, 33, 0.5, "mean", "mixed", seed=1)
    ids, m1, m2 = case.batches(1)[0]
    args = (case.state0(), *case.store, ids, m1, m2, 0.5, "mean")
    _, g64, _ = R.loss_and_grads(*args)
    a = R.loss_and_grads(*args, R.Sums(np.float32, np.random.default_rng(1)))[1]
    b = R.loss_and_grads(*args, R.Sums(np.float32, np.random.default_rng(2)))[1]
    assert a["W1"].dtype == np.float32 and not np.array_equal(a["W1"], b["W1"])
    assert np.max(np.abs(a["W1"] - g64["W1"])) < 1e-5 * np.max(np.abs(g64["W1"]))


# ---- layouts and inputs --------------------------------------------------------------------------------------------
def test_shape_list_reaches_every_layout(signnet):
    seen = set()
    for H, IW, B, p, mode, kind in K.SHAPES:
        lay = signnet.layout(H, IW, B, pooled=bool(mode))
        assert lay["columns_per_workgroup"] * lay["workgroups"] >= H > lay["columns_per_workgroup"] * (lay["workgroups"] - 1)
        assert lay["k_tile"] == 64 * lay["k_vector"] and lay["row_tile"] == R.ROW_TILE == lay["score_tile"]
        seen.add((lay["k_vector"], lay["head_k_vector"]))
    every = set()
    for H in (1, 2, 3, 4):
        for IW in (1, 2, 3, 4):
            for pooled in (False, True):
                lay = signnet.layout(H, IW, 2, pooled)
                every.add((lay["k_vector"], lay["head_k_vector"]))
    assert every == K.LAYOUTS == seen
    Hs, Ws, Bs, ps, modes, kinds = (set(s[i] for s in K.SHAPES) for i in range(6))
    assert {1, 2, 7, 32, 33, 64, 255, 256} <= Hs and {1, 3, 64, 65, 260, 2004} <= Ws and {2, 3, 32, 33, 64} <= Bs
    assert ps == {0.0, 0.5} and modes == {"", "mean", "sum"} and kinds == {"two", "mixed"}
    assert signnet.layout(8, 256, 2)["k_tile"] + 4 == 260 and signnet.layout(8, 65, 2)["k_tile"] + 1 == 65
    assert max(s[0] for s in K.SHAPES) > signnet.layout(256, 8, 2)["columns_per_workgroup"]      # more than one block
    x, row_ptr, _ = K.make_store("mixed", 3, 0)
    cnt = np.diff(row_ptr)
    assert cnt.max() == K.BIG_ROWS > R.ROW_TILE and cnt[0] == cnt[-1] == 2 and {2, 3} <= set(cnt)
    ids = K.batch_ids(33, np.random.default_rng(0))
    assert ids[0] == K.NUM_LINKS - 1 and 0 in ids and K.BIG_LINK in ids and len(set(ids)) == 33
    assert (np.diff(ids) < 0).any() and (np.diff(ids) > 0).any()


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_recorded_seeds_meet_the_conditions(shape):
    H, IW, B, p, mode, kind = shape
    case = K.Case(H, IW, B, p, mode, kind, K.SEEDS[shape])
    st = case.state0()
    for ids, m1, m2 in case.batches(3):
        st, _, _, f = R.step(st, *case.store, ids, m1, m2, p, mode, case.lr)
        var, margin = K.conditions(f)
        assert var >= K.MIN_VARIANCE and margin >= K.RELU_MARGIN


# ---- faults --------------------------------------------------------------------------------------------------------
def test_every_fault_lands_far_outside_the_bounds():
    """Each fault's worst |faulty - restatement| / bound over the state and the loss, after one clean step so that the
    moments are non-zero: H = 32, in_width = 64, B = 33 of the mixed store ("mean"), 137 rows, so three row tiles."""
    H, IW, B, p, mode, lr = 32, 64, 33, 0.5, "mean", 1e-3
    case = K.Case(H, IW, B, p, mode, "mixed", seed=1, lr=lr)
    x, row_ptr, y = case.store
    (ids0, a1, a2), (ids, m1, m2) = case.batches(2)
    st = R.step(case.state0(), x, row_ptr, y, ids0, a1, a2, p, mode, lr)[0]
    assert (np.diff(row_ptr)[ids] == 2).any() and (row_ptr[ids + 1] - row_ptr[ids]).sum() > 2 * R.ROW_TILE
    clean, loss, bounds, _ = K.step_bounds(st, x, row_ptr, y, ids, m1, m2, p, mode, lr)
    factors = {}
    for fault in R.FAULTS:
        bad, bad_loss, _, _ = R.step(st, x, row_ptr, y, ids, m1, m2, p, mode, lr, fault=fault)
        r = K.worst_ratio(bad, clean, bounds)
        r["loss"] = abs(bad_loss - loss) / bounds["loss"]
        factors[fault] = max(r.values())
    print({k: f"{v:.1e}" for k, v in factors.items()})
    assert all(v >= 10 for v in factors.values()), factors
    assert max(K.worst_ratio(clean, clean, bounds).values()) == 0.0


# ---- arguments -----------------------------------------------------------------------------------------------------
def test_argument_checks(signnet):
    T = signnet.SIGNNetTrainer
    with pytest.raises(NotImplementedError, match="concat"):
        T(12, 8, k_heuristic=2, k_pool_strategy="concat")
    with pytest.raises(NotImplementedError, match="256"):
        T(12, 257)
    with pytest.raises(NotImplementedError, match="1048576"):
        T((1 << 20) + 1, 8)
    with pytest.raises(NotImplementedError, match="64"):
        signnet.layout(8, 12, 65)
    with pytest.raises(ValueError, match="two links"):
        signnet.layout(8, 12, 1)
    with pytest.raises(NotImplementedError, match="pool strat"):
        T(12, 8, k_heuristic=1, k_pool_strategy="max")
    for bad in (dict(hidden=0), dict(in_width=0), dict(dropout=1.0), dict(dropout=-0.1), dict(lr=0.0),
                dict(lr=float("nan"))):
        kw = dict(in_width=12, hidden=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            T(**kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T(12, 8, device="cpu")
    sd = K.twin_state_dict(K.init_params(8, 12, 1, 0))
    with pytest.raises(ValueError, match="lacks"):
        T(12, 8, init={k: v for k, v in sd.items() if k != "link_pred_mlp.4.bias"})
    with pytest.raises(ValueError, match="must be"):
        T(13, 8, init=sd)
    for ids, msg in ((np.zeros(3), "integer"), (np.array([0, 10]), "outside"), (np.array([-1, 0]), "outside"),
                     (np.zeros((2, 2), dtype=np.int64), r"\[B\]")):
        with pytest.raises(ValueError, match=msg):
            signnet._link_ids(ids, 10)
    from s3grl_amd.harness import SIGNNetTwin

    assert list(SIGNNetTwin(12, 8, 1, "mean").state_dict()) == list(signnet.STATE_ORDER)
    assert signnet.PARAM_KEYS == K.PARAM_KEYS


# ---- must fail without the feature ---------------------------------------------------------------------------------
def test_signnet_is_part_of_the_abi(signnet):
    from s3grl_amd import _native, harness

    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_signnet_[a-z_]+)\s*\(", header))
    assert declared == {"s3grl_signnet_" + n for n in ("layout", "create", "fit_epoch", "draws", "step", "score",
                                                       "read_state", "write_state", "destroy")}
    assert declared <= set(_native.SYMBOLS)
    for name in declared:
        assert getattr(_native.lib(), name) is not None
    import s3grl_amd

    assert callable(s3grl_amd.SIGNNetTrainer) and callable(harness.train_and_evaluate_fused)
    assert "s3grl_signnet.hip" in __import__("__graft_entry__").SOURCES
