"""Host-side checks of the SAGE / GIN work (no GPU): the restatement tests/mpnn_reference.py on a hand-computed graph,
the twins' state_dict keys, argument errors raised before any GPU work, the harness boundary and the C ABI names."""
import pytest
import torch

from mpnn_reference import (aggregate_mean, aggregate_mean_t, aggregate_mean_t_wrong_side, aggregate_sum,
                            aggregate_sum_t, segment_mean)

# 5 nodes: 0 -> 1 twice (a duplicated arc), 1 -> 1 (an input self-loop), 2 -> 3 (one way only), 3 -> 0; 4 is isolated
SRC = torch.tensor([0, 0, 1, 2, 3])
DST = torch.tensor([1, 1, 1, 3, 0])
H = torch.tensor([[1.0, -1.0], [2.0, -2.0], [4.0, -4.0], [8.0, -8.0], [16.0, -16.0]], dtype=torch.float64)


def _col(values):
    v = torch.tensor(values, dtype=torch.float64)
    return torch.stack([v, -v], 1)


def test_restatement_sum_and_mean_by_hand():
    # into 0: h3; into 1: h0 + h0 + h1; into 3: h2; nothing into 2 and 4
    assert torch.equal(aggregate_sum(H, SRC, DST), _col([8, 4, 0, 4, 0]))
    # in-degrees 1, 3, 0, 1, 0; a node without in-arcs gets zero, never NaN
    torch.testing.assert_close(aggregate_mean(H, SRC, DST), _col([8, 4 / 3, 0, 4, 0]), rtol=1e-15, atol=0)


def test_restatement_transposes_by_hand():
    # out of 0: g1 twice; out of 1: g1; out of 2: g3; out of 3: g0
    assert torch.equal(aggregate_sum_t(H, SRC, DST), _col([4, 2, 8, 1, 0]))
    # each arc weighted by 1 / indeg of its DESTINATION: node 1 has in-degree 3
    torch.testing.assert_close(aggregate_mean_t(H, SRC, DST), _col([4 / 3, 2 / 3, 8, 1, 0]), rtol=1e-15, atol=0)
    # weighting by the row's own degree instead is a different operator on this graph
    assert not torch.allclose(aggregate_mean_t_wrong_side(H, SRC, DST), aggregate_mean_t(H, SRC, DST))
    # the transposes are the adjoints: <A h, g> = <h, A^T g>
    g = torch.randn(5, 2, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    for fwd, bwd in ((aggregate_sum, aggregate_sum_t), (aggregate_mean, aggregate_mean_t)):
        torch.testing.assert_close((fwd(H, SRC, DST) * g).sum(), (H * bwd(g, SRC, DST)).sum())


def test_restatement_segment_mean_by_hand():
    out = segment_mean(H, torch.tensor([0, 2, 2, 5]))             # sizes 2, 0 (empty), 3
    torch.testing.assert_close(out, _col([1.5, 0, 28 / 3]), rtol=1e-15, atol=0)


def test_twin_state_dict_keys_and_shapes():
    from s3grl_amd.mpnn import GINTwin, SAGETwin

    s = SAGETwin(32, 3, 1000).state_dict()
    assert [k for k in s if k.startswith("convs.")] == [
        f"convs.{i}.{k}" for i in range(3) for k in ("lin_l.weight", "lin_l.bias", "lin_r.weight")]
    assert s["convs.0.lin_l.weight"].shape == (32, 32) and s["convs.2.lin_r.weight"].shape == (32, 32)
    assert s["z_embedding.weight"].shape == (1000, 32) and s["mlp.lins.0.weight"].shape == (32, 32)
    assert s["mlp.lins.1.weight"].shape == (1, 32) and s["mlp.norms.0.running_var"].shape == (32,)
    for jk, width in ((True, 96), (False, 32)):
        g = GINTwin(32, 3, 1000, jk=jk).state_dict()
        body = ["nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias", "nn.4.weight", "nn.4.bias",
                "nn.4.running_mean", "nn.4.running_var", "nn.4.num_batches_tracked"]
        for p in ("conv1", "convs.0", "convs.1"):
            assert [k for k in g if k.startswith(p + ".")] == [f"{p}.eps"] + [f"{p}.{k}" for k in body]
            assert g[p + ".eps"].shape == (1,) and float(g[p + ".eps"]) == 0.0
        assert "convs.2.eps" not in g
        assert g["mlp.lins.0.weight"].shape == (32, width)
    t = GINTwin(16, 2, 50, train_eps=True)
    assert isinstance(t.conv1.eps, torch.nn.Parameter) and "conv1.eps" in t.state_dict()
    assert not isinstance(GINTwin(16, 2, 50).conv1.eps, torch.nn.Parameter)


def test_net_twin_state_dict_keys_and_init():
    from s3grl_amd.mpgnn import NetTwin

    keys = {"GCN": ["bias", "lin.weight"], "SAGE": ["lin_l.weight", "lin_l.bias", "lin_r.weight"],
            "GIN": ["eps", "nn.0.weight", "nn.0.bias", "nn.2.weight", "nn.2.bias"]}
    for layer, ks in keys.items():
        net = NetTwin(7, 32, layer, seed=3)
        sd = net.state_dict()
        assert list(sd) == [f"conv{i}.{k}" for i in (1, 2, 3) for k in ks]
        first = {"GCN": "conv1.lin.weight", "SAGE": "conv1.lin_l.weight", "GIN": "conv1.nn.0.weight"}[layer]
        assert sd[first].shape == (32, 7)
        again = NetTwin(7, 32, layer, seed=3).state_dict()
        assert all(torch.equal(sd[k], again[k]) for k in sd)          # the seed decides the init
        assert not torch.equal(sd[first], NetTwin(7, 32, layer, seed=4).state_dict()[first])
    sd = NetTwin(7, 32, "SAGE", seed=0).state_dict()
    assert float(sd["conv1.lin_l.weight"].abs().max()) <= 7 ** -0.5   # torch's Linear bound 1 / sqrt(in)
    assert float(sd["conv2.lin_l.bias"].abs().max()) <= 32 ** -0.5
    with pytest.raises(NotImplementedError):
        NetTwin(7, 32, "GAT")


def test_argument_errors_before_gpu_work():
    from s3grl_amd import mpgnn
    from s3grl_amd.mpnn import GINTwin, SAGETwin, aggregate, segment_mean as hip_segment_mean

    for twin in (SAGETwin, GINTwin):
        with pytest.raises(NotImplementedError):
            twin(32, 3, 1000, dropedge=0.2)
        with pytest.raises(NotImplementedError):
            twin(32, 3, 1000, node_embedding=torch.nn.Embedding(4, 2))
        with pytest.raises(ValueError):
            twin(32, 3, 1000, use_feature=True)                       # no features to size the first layer
    with pytest.raises(ValueError, match="mode"):
        aggregate(torch.zeros(3, 2), None, "max")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aggregate(torch.zeros(3, 2), None, "sum")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_segment_mean(torch.zeros(3, 2), torch.tensor([0, 3]))
    lists = [torch.zeros((2, 1), dtype=torch.int64)] * 5
    with pytest.raises(NotImplementedError):
        mpgnn.train(torch.zeros((2, 1), dtype=torch.int64), None, lists, "GAT", num_nodes=3)
    with pytest.raises(ValueError, match="num_nodes"):
        mpgnn.train(torch.zeros((2, 1), dtype=torch.int64), None, lists, "SAGE")
    with pytest.raises(ValueError, match="split_lists"):
        mpgnn.train(torch.zeros((2, 1), dtype=torch.int64), None, lists[:4], "SAGE", num_nodes=3)
    with pytest.raises(ValueError, match="outside"):
        mpgnn.train(torch.tensor([[0], [5]]), None, lists, "GIN", num_nodes=3)


def test_harness_boundary():
    from s3grl_amd.harness import train_and_evaluate_seal, train_and_evaluate_seal_mpnn

    with pytest.raises(NotImplementedError):
        train_and_evaluate_seal_mpnn((None, None), (None, None), model="DGCNN")
    with pytest.raises(NotImplementedError):
        train_and_evaluate_seal((None, None), (None, None), model="SAGE")


def test_native_symbols_list_the_new_calls():
    from s3grl_amd import _native

    for name in ("s3grl_nbr_aggregate", "s3grl_segment_mean_forward", "s3grl_segment_mean_backward"):
        assert name in _native.SYMBOLS
    assert (_native.SCALE_NONE, _native.SCALE_OWN, _native.SCALE_NEIGHBOUR) == (0, 1, 2)
    assert _native.ABI_VERSION == 6
