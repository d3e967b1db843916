"""Host-side checks of the graph autoencoders (s3grl_amd.gae, tests/gae_reference.py): the pair-key mapping, the
restated loss and its gradient, the KL switch, the reference's model selection and the refusals.  No GPU needed."""
import re
from itertools import product
from pathlib import Path

import numpy as np
import pytest
import torch

import gae_reference as R
from s3grl_amd import gae

REPO = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6])
def test_pair_key_round_trips_exhaustively(n):
    pairs = [(i, j) for i, j in product(range(n), range(n)) if i != j]
    i = torch.tensor([p[0] for p in pairs])
    j = torch.tensor([p[1] for p in pairs])
    k = R.pair_key(i, j, n)
    assert sorted(k.tolist()) == list(range(n * (n - 1)))          # a bijection onto [0, N(N-1))
    assert torch.equal(k, torch.sort(k).values)                      # ordered by (i, j)
    i2, j2 = R.pair_of_key(torch.arange(n * (n - 1)), n)
    assert torch.equal(i2, i) and torch.equal(j2, j)


def _toy(seed=0, n=9, emb=4):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn((n, emb), generator=g, dtype=torch.float64)
    pos = torch.tensor([[0, 1, 2, 3, 4, 1, 2], [1, 0, 3, 2, 5, 2, 1]])
    neg = torch.tensor([[0, 5, 7, 8, 6], [7, 3, 8, 2, 0]])
    return z, pos, neg


def test_restated_loss_gradient_matches_autograd():
    z, pos, neg = _toy()
    lg = torch.cat([R.logits(z, pos), R.logits(z, neg)]).requires_grad_(True)
    P = pos.shape[1]
    loss = -torch.log(torch.sigmoid(lg[:P]) + R.EPS).mean() - torch.log(1 - torch.sigmoid(lg[P:]) + R.EPS).mean()
    loss.backward()
    assert torch.allclose(R.recon_coef(z, pos, neg), lg.grad, rtol=1e-12, atol=0)
    assert torch.allclose(R.recon_loss(z, pos, neg), loss.detach(), rtol=1e-14)


def _state(model, n=9, hidden=6, emb=4, seed=3):
    return {k: v.detach() for k, v in gae.TWINS[model](n, emb, hidden, seed=seed).state_dict().items()}


@pytest.mark.parametrize("model", ["VGAE", "ARGVA"])
def test_kl_term_only_when_regularised(model):
    z, pos, neg = _toy()
    n = 9
    sd = _state(model)
    noise = torch.randn((n, 4), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    plain = R.training_loss(sd, None, pos, n, model, neg, noise)
    zz, mu, logstd = R.encode(sd, None, pos, n, model, noise)
    assert torch.equal(plain, R.recon_loss(zz, pos, neg))           # as written: no KL
    reg = R.training_loss(sd, None, pos, n, model, neg, noise, regularise=True)
    assert int(pos.max()) == 5
    assert torch.allclose(reg - plain, R.kl_loss(mu, logstd) / 5, rtol=1e-12, atol=1e-15)


def test_gae_has_no_kl_even_when_regularised():
    z, pos, neg = _toy()
    sd = _state("GAE")
    assert torch.equal(R.training_loss(sd, None, pos, 9, "GAE", neg, regularise=True),
                       R.training_loss(sd, None, pos, 9, "GAE", neg))


def test_twin_parameters_are_glorot_and_zero_bias():
    sd = _state("VGAE", n=50, hidden=20, emb=10)
    a = (6.0 / (50 + 20)) ** 0.5
    w = sd["encoder.conv1.lin.weight"]
    assert w.shape == (20, 50) and float(w.abs().max()) <= a and float(w.std()) > a / 3
    assert sd["encoder.conv_mu.lin.weight"].shape == (10, 20)
    assert all(float(sd[k].abs().max()) == 0 for k in sd if k.endswith(".bias"))
    assert torch.equal(w, _state("VGAE", n=50, hidden=20, emb=10)["encoder.conv1.lin.weight"])   # seeded


@pytest.mark.parametrize("results", [
    [(0.5, 0.1), (0.9, 0.2), (0.9, 0.3), (0.7, 0.4)],      # tie: the first maximum
    [(0.9, 0.6), (0.8, 0.2), (0.9, 0.3)],
    [(0.3, 0.3)],
    [(0.1, 0.9), (0.2, 0.8), (0.3, 0.7)],
])
def test_best_test_at_first_max_val(results):
    assert gae.best_at_first_max(results) == pytest.approx(R.best_at_first_max(results))
    val, test = gae.best_at_first_max(results)
    first = next(i for i, r in enumerate(results) if r[0] == max(x[0] for x in results))
    assert (val, test) == results[first]


class _Args:
    epochs, embedding_dim, hidden_channels, lr, eval_steps, log_steps, res_dir = 2, 4, 8, 0.01, 1, 1, ""


def _lists():
    return [np.array([[0], [1]]), np.array([[2], [3]]), np.array([[1], [2]]), np.array([[0], [3]])]


def test_refuses_unknown_model():
    with pytest.raises(NotImplementedError):
        gae.run_vgae(np.array([[0, 1], [1, 0]]), torch.eye(4), _lists(), "GIC", _Args())


def test_refuses_cpu_device():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gae.run_vgae(np.array([[0, 1], [1, 0]]), torch.eye(4), _lists(), "GAE", _Args(), device="cpu")


def test_refuses_ids_outside_graph():
    with pytest.raises(ValueError, match="outside"):
        gae.run_vgae(np.array([[0, 4], [4, 0]]), torch.eye(4), _lists(), "GAE", _Args(), device="cpu")
    bad = _lists()
    bad[1] = np.array([[-1], [2]])
    with pytest.raises(ValueError, match="outside"):
        gae.run_vgae(np.array([[0, 1], [1, 0]]), torch.eye(4), bad, "VGAE", _Args(), device="cpu")


def test_refuses_wrong_feature_rows():
    class Split:
        num_nodes = 5
        links = {"train": (np.array([[0, 1], [1, 0]]), None), "valid": _lists()[2:], "test": _lists()[:2]}

        def edge_index(self):
            return self.links["train"][0]

    with pytest.raises(ValueError, match="rows"):
        gae.run_gae(Split(), "GAE", x=torch.ones(4, 3), device="cpu")


def test_new_symbols_declared_and_bound():
    from s3grl_amd import _native

    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_gae_[a-z_]+)\s*\(", header))
    assert declared == {"s3grl_gae_keys", "s3grl_gae_negatives", "s3grl_gae_incidence", "s3grl_gae_decode",
                        "s3grl_gae_backward"}
    assert declared <= set(_native.SYMBOLS)
    assert "s3grl_gae.hip" in (REPO / "__graft_entry__.py").read_text()
