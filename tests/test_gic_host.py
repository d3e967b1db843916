"""Graph InfoClust on the host: the restatement of tests/gic_reference.py against the reference-pinned golden files,
the pure arc / coefficient builder of `GicGraph`, the hyper-parameter table and the argument checks."""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import gic_reference as R  # noqa: E402
from s3grl_amd import gic  # noqa: E402
from s3grl_amd.propagate import add_remaining_self_loops, gic_arcs  # noqa: E402


@pytest.mark.parametrize("case", R.CASES)
def test_restatement_reproduces_golden(case):
    g, out = R.restated(case)
    keys = [k for k in g if k in R.OUTPUTS or k.startswith("g_")]
    assert {"g_" + k for k in R.PARAMS} <= set(keys) and set(R.OUTPUTS) <= set(keys)
    for k in keys:
        if k.endswith("_rows"):
            continue
        err = R.rel(R.stored(g, k, out[k]), g[k])
        assert err < 1e-9, (k, err)


@pytest.mark.parametrize("case", R.CASES)
def test_golden_is_finite_and_small(case):
    g = R.golden(case)
    assert all(np.isfinite(v).all() for v in g.values() if v.dtype.kind == "f")
    assert (Path(R.__file__).parent / "golden" / f"gic_{case}.npz").stat().st_size < 1_000_000


def _dense_of_arcs(src, dst, coef, n):
    M = torch.zeros((n, n), dtype=torch.float64)
    M.index_put_((dst, src), coef, accumulate=True)      # out[dst] += coef · h[src]
    return M


@pytest.mark.parametrize("case", ["tiny", "rand300", "usair"])
def test_builder_reproduces_golden_operator(case):
    g = R.golden(case)
    n = int(g["num_nodes"])
    arcs = torch.as_tensor(g["arcs"]).long()
    src, dst, coef = gic_arcs(arcs[:, 0], arcs[:, 1], n)
    assert coef.dtype == torch.float64 and src.numel() == arcs.shape[0] + n
    want = R.dense((g["op_row"], g["op_col"], g["op_val"]), n)
    assert R.rel(_dense_of_arcs(src, dst, coef, n), want) < 1e-14
    assert R.rel(R.dense(R.operator(g["arcs"].T, n), n), want) < 1e-14


def test_operator_is_not_gcn_on_tiny():
    g = R.golden("tiny")
    n = int(g["num_nodes"])
    arcs = torch.as_tensor(g["arcs"]).long()
    s, t, _ = add_remaining_self_loops(arcs[:, 0], arcs[:, 1], None, n)
    dinv = torch.bincount(t, minlength=n).double().pow(-0.5)          # gcn_norm: in-degree with the loop
    gcn = _dense_of_arcs(s, t, dinv[s] * dinv[t], n)
    ours = _dense_of_arcs(*gic_arcs(arcs[:, 0], arcs[:, 1], n), n)
    assert R.rel(ours, gcn) > 0.05
    assert float(ours[3, 3]) == pytest.approx(1.0)                    # (A + I)[3, 3] = 2 and rowsum 2: the loop is kept
    assert float(ours[1, 0]) == pytest.approx(1.0 / 3.0)             # arc 0 -> 1: out-degrees 2 and 2, each + 1
    assert float(ours[5, 5]) == pytest.approx(1.0)                    # the isolated node


def test_operator_equals_gcn_on_a_symmetric_graph():
    arcs = torch.tensor([[0, 1], [1, 0], [1, 2], [2, 1], [0, 3], [3, 0]])
    n = 5
    s, t, _ = add_remaining_self_loops(arcs[:, 0], arcs[:, 1], None, n)
    dinv = torch.bincount(t, minlength=n).double().pow(-0.5)
    assert R.rel(_dense_of_arcs(*gic_arcs(arcs[:, 0], arcs[:, 1], n), n),
                 _dense_of_arcs(s, t, dinv[s] * dinv[t], n)) < 1e-15


def test_hyper_parameters():
    assert gic.hyper_parameters("cora") == (100, 0.5, 128)
    assert gic.hyper_parameters("citeseer") == (100, 0.5, 128)
    assert gic.hyper_parameters("pubmed") == (10, 0.75, 32)
    assert gic.hyper_parameters("usair") == (100, 0.5, 10)
    assert gic.hyper_parameters("anything") == (100, 0.5, 10)
    for name in ("cora", "pubmed", "usair"):
        assert gic.hyper_parameters(name) == R.hyper_parameters(name)
    assert gic.PATIENCE == 100 and gic.DETACHED_ITERS == 10


def test_twin_initialisation():
    net = gic.GICTwin(50, 7, 12, 4, 100, seed=3)
    sd = net.state_dict()
    assert set(sd) == set(R.PARAMS) | {"init"}
    assert {n for n, _ in net.named_parameters()} == set(R.PARAMS)    # init is a buffer: never trained
    assert sd["gcn.fc.weight"].abs().max() <= (6 / 19) ** 0.5 and sd["disc.f_k.weight"].abs().max() <= (6 / 156) ** 0.5
    assert not sd["gcn.bias"].any() and not sd["disc.f_k.bias"].any() and float(sd["gcn.act.weight"]) == 0.25
    assert sd["init"].shape == (4, 12) and 0 <= sd["init"].min() and sd["init"].max() < 1
    ref = R.init_state(7, 12, 4, 3)
    assert all(torch.equal(sd[k], ref[k]) for k in sd)


def test_shape_limits_and_bad_ids_raise():
    from s3grl_amd import _native

    with pytest.raises(ValueError, match=str(_native.GIC_MAX_CLUSTERS)):
        gic.check_shape(10, 32, _native.GIC_MAX_CLUSTERS + 1)
    with pytest.raises(ValueError, match=str(_native.GIC_MAX_DIM)):
        gic.check_shape(10, _native.GIC_MAX_DIM + 1, 10)
    with pytest.raises(ValueError):
        gic.check_shape(0, 32, 10)
    gic.check_shape(1, 512, 256)
    ei = torch.tensor([[0, 1], [1, 2]])
    lists = [ei, ei, ei, ei]
    kw = dict(epochs=1, lr=0.01, eval_steps=1)
    with pytest.raises(ValueError, match=str(_native.GIC_MAX_DIM)):
        gic.train(ei, None, "usair", lists, embedding_dim=_native.GIC_MAX_DIM + 1, num_nodes=3, **kw)
    with pytest.raises(ValueError, match="outside"):
        gic.train(torch.tensor([[0, 3], [1, 2]]), None, "usair", lists, embedding_dim=8, num_nodes=3, **kw)
    with pytest.raises(ValueError, match="outside"):
        gic.train(ei, torch.zeros(3, 2), "usair", [ei, ei, ei, torch.tensor([[0], [-1]])], embedding_dim=8, **kw)
    with pytest.raises(ValueError):
        gic.train(ei, None, "usair", lists, embedding_dim=8, **kw)               # eye features need num_nodes


def test_no_cpu_fallback():
    ei = torch.tensor([[0, 1], [1, 2]])
    args = SimpleNamespace(epochs=1, lr=0.01, embedding_dim=8, eval_steps=1, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gic.CalGIC(ei, torch.eye(3), "usair", [ei, ei, ei, ei], args, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gic.clusterator(torch.zeros(3, 4), torch.ones(2, 4), 10.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gic.cluster_discriminator(torch.zeros(3, 2), torch.zeros(2, 4), torch.zeros(3, 4), torch.zeros(3, 4))


def test_step_rule_of_the_restatement():
    g = R.golden("tiny")
    x, _, _, n, _, _ = R.golden_inputs(g)
    lists = [torch.tensor([[0, 1], [1, 2]])] * 4
    _, _, trace = R.train_loop(g["arcs"].T, x, n, lists, "pubmed", epochs=6, lr=0.01, dim=5, seed=0)
    best, want = 1e9, []
    for e, v in enumerate(trace["loss"]):
        if v < best:
            best = v
        else:
            want.append(e)
    assert trace["stepped"] == want and 0 not in trace["stepped"]
    _, _, every = R.train_loop(g["arcs"].T, x, n, lists, "pubmed", epochs=6, lr=0.01, dim=5, seed=0,
                               step_every_epoch=True)
    assert every["stepped"] == list(range(6))
