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


# ---- the restated negative sampling and pair backward ---------------------------------------------------------------
_M64 = (1 << 64) - 1
_GOLDEN = 0x9e3779b97f4a7c15   # splitmix64's increment: mix(k · _GOLDEN) is the k-th output of splitmix64 seeded 0


def test_mix64_against_values_worked_by_hand():
    # the published first three outputs of splitmix64 with seed 0
    assert int(R.mix64(_GOLDEN)) == 0xe220a8397b1dcdaf
    assert int(R.mix64((2 * _GOLDEN) & _M64)) == 0x6e789e6aa1b965f4
    assert int(R.mix64((3 * _GOLDEN) & _M64)) == 0x06c45d188009454f
    assert int(R.mix64(0)) == 0
    # x = 1, every step in Python integers
    x = 1
    x = x ^ (x >> 30)                                   # 1: the shift gives 0
    assert x == 1
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    assert x == 0xbf58476d1ce4e5b9
    x = x ^ (x >> 27)                                   # the top 37 bits, 0x17eb08eda3, onto the low ones
    assert x == 0xbf58477af7ec081a
    x = (x * 0x94d049bb133111eb) & _M64
    assert x == 0x5692161dbd2f29de
    x = x ^ (x >> 31)                                   # 0xad242c3b
    assert x == 0x5692161d100b05e5
    assert int(R.mix64(1)) == x
    got = R.mix64(np.array([_GOLDEN, 1, 0], dtype=np.uint64))      # vectorised: the same values
    assert [int(v) for v in got] == [0xe220a8397b1dcdaf, x, 0]


def test_mulhi64_is_the_high_word_of_the_product():
    a = [0, 1, _M64, 1 << 63, (1 << 32) - 1, 1 << 32, 0x123456789abcdef0, 0xe220a8397b1dcdaf]
    for b in (1, 20, (1 << 32) - 1, 1 << 32, 70000 * 69999, 235000 * 234999, _M64):
        got = R.mulhi64(np.array(a, dtype=np.uint64), b)
        assert [int(v) for v in got] == [(x * b) >> 64 for x in a]
    # a draw lands in [0, pop): the largest hash gives pop − 1
    assert int(R.mulhi64(np.array([_M64], dtype=np.uint64), 20)[0]) == 19


def _mix_py(x):
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & _M64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & _M64
    return x ^ (x >> 31)


def _rounds_py(n, S, seed, epoch):
    """The three rounds of S draws in Python integers (no numpy, not R's helpers)."""
    key = _mix_py(_mix_py(_mix_py(seed & 0xffffffff) ^ epoch) ^ 0x6761655f6e6567)
    pop = n * (n - 1)
    return [[(_mix_py(key ^ _mix_py((r << 40) ^ i)) * pop) >> 64 for i in range(S)] for r in range(3)]


def _positives(n, m, seed):
    return np.sort(np.random.default_rng(seed).choice(n * (n - 1), m, replace=False)).astype(np.int64)


@pytest.mark.parametrize("seed,epoch", [(0, 0), (0, 1), (3, 0), (5, 2), (2 ** 35 + 3, 0)])
@pytest.mark.parametrize("count", [1, 3, 6])
def test_negatives_on_five_nodes_by_brute_force_over_all_keys(seed, epoch, count):
    n, pop = 5, 20
    pos = _positives(n, 8, 1)
    S = int(1.1 * count / (1.0 - 8 / 20))
    assert 1 <= S < pop                                            # sparse mode
    flat = [k for r in _rounds_py(n, S, seed, epoch) for k in r]
    # by key, not by walk: every free key's earliest draw; the `count` keys of the earliest such draws
    first = {k: flat.index(k) for k in range(pop) if k not in set(pos.tolist()) and k in flat}
    want = sorted(sorted(first, key=first.get)[:count])
    trace = {}
    got = R.negatives(pos, n, count, seed, epoch, trace)
    assert got.dtype == torch.int64 and got.tolist() == want
    assert trace["S"] == S and trace["T"] == 3 * S and not trace["enumerate"]
    assert sum(trace["kept_per_round"]) == len(want)
    if seed >= 2 ** 32:                                            # the seed counts modulo 2^32
        assert torch.equal(got, R.negatives(pos, n, count, seed % 2 ** 32, epoch))


def test_negatives_enumerate_mode_is_the_complement_of_the_positives():
    n, pop = 5, 20
    pos = _positives(n, 8, 2)
    free = sorted(set(range(pop)) - set(pos.tolist()))
    for count in (11, 12, 40):                                     # 1.1·11 / 0.6 = 20.17 >= 20
        trace = {}
        got = R.negatives(pos, n, count, 9, 4, trace)
        assert trace["enumerate"] and trace["S"] == pop == trace["T"]
        assert got.tolist() == free[:count]
        assert torch.equal(got, R.negatives(pos, n, count, 1, 0))  # no draw is random
    trace = {}
    R.negatives(pos, n, 10, 9, 4, trace)                           # 1.1·10 / 0.6 = 18.3 < 20
    assert not trace["enumerate"] and trace["S"] == 18
    # duplicated positives count in M (PyG's idx.numel()) but not twice as keys
    dup = np.concatenate([pos, pos[:3]])
    R.negatives(dup, n, 10, 9, 4, trace)
    assert trace["enumerate"]                                      # 1.1·10 / (1 − 11/20) = 24.4
    assert R.negatives(np.arange(pop), n, 5, 0, 0).numel() == 0    # no room for a negative
    assert R.negatives(pos, n, 0, 0, 0).numel() == 0


def _pyg_rounds(rounds, pos, count):
    """PyG 2.0.x negative_sampling's loop over given rounds of draws (each round's draws distinct)."""
    idx, neg = np.asarray(pos), None
    for rnd in rounds:
        rnd = np.asarray(rnd, dtype=np.int64)
        mask = np.isin(rnd, idx)
        if neg is not None:
            mask |= np.isin(rnd, neg)
        rnd = rnd[~mask]
        neg = rnd if neg is None else np.concatenate([neg, rnd])
        if neg.size >= count:
            neg = neg[:count]
            break
    return neg


@pytest.mark.parametrize("seed,epoch,short", [(0, 0, True), (4, 1, True), (1, 0, False)])
def test_negatives_follow_pyg_rounds_when_round_one_falls_short(seed, epoch, short):
    n, count = 8, 14
    pos = _positives(n, 30, 1)
    S = int(1.1 * count / (1.0 - 30 / 56))
    rounds = [list(dict.fromkeys(r)) for r in _rounds_py(n, S, seed, epoch)]   # a round without its repeats
    want = _pyg_rounds(rounds, pos, count)
    trace = {}
    got = R.negatives(pos, n, count, seed, epoch, trace)
    assert got.tolist() == sorted(want.tolist()) and len(got) == count
    assert (trace["kept_per_round"][0] < count) == short           # the case is what it claims to be
    if short:
        assert trace["kept_per_round"][1] > 0 and sum(trace["kept_per_round"]) == count


def test_pair_backward_matches_autograd_with_self_and_duplicate_pairs():
    g = torch.Generator().manual_seed(5)
    z = torch.randn((7, 3), generator=g, dtype=torch.float64, requires_grad=True)
    pairs = torch.tensor([[0, 1, 2, 2, 0, 4, 4], [1, 0, 2, 2, 1, 5, 4]])   # self pairs, duplicates; node 3, 6 in none
    coef = torch.randn(7, generator=g, dtype=torch.float64)
    (R.logits(z, pairs) * coef).sum().backward()
    got = R.pair_backward(z.detach(), pairs, coef)
    assert torch.allclose(got, z.grad, rtol=1e-13, atol=1e-15)
    assert torch.equal(got[3], torch.zeros(3, dtype=torch.float64)) and not got[6].any()
    assert torch.allclose(got[4], coef[5] * z[5].detach() + 2 * coef[6] * z[4].detach(), rtol=1e-13)
