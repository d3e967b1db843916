"""CPU checks of the SEAL models' operators: hand-computed gcn_norm answers and sort-pool order in the restatement
(tests/seal_nn_reference.py), the reference's sortpool_k rule, and the argument checks of s3grl_amd.seal_nn that
refuse before any GPU work."""
import math

import pytest
import torch

from seal_nn_reference import gcn_norm, propagate, sort_pool


def coef_of(src, dst, coef):
    return {(int(a), int(b)): float(c) for a, b, c in zip(src, dst, coef)}


def test_gcn_norm_path_graph():
    # 0 - 1 - 2 both directions: deg with loop = 2, 3, 2
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    c = coef_of(*gcn_norm(ei, 3))
    assert len(c) == 7
    assert c[(0, 0)] == pytest.approx(1 / 2) and c[(1, 1)] == pytest.approx(1 / 3) and c[(2, 2)] == pytest.approx(1 / 2)
    assert c[(0, 1)] == pytest.approx(1 / math.sqrt(6)) and c[(1, 0)] == pytest.approx(1 / math.sqrt(6))
    assert c[(2, 1)] == pytest.approx(1 / math.sqrt(6))
    h = torch.tensor([[1.0], [2.0], [4.0]], dtype=torch.float64)
    out = propagate(h, *gcn_norm(ei, 3))
    assert out[1, 0] == pytest.approx(1 / math.sqrt(6) + 2 / 3 + 4 / math.sqrt(6))


def test_gcn_norm_existing_self_loop_keeps_its_weight():
    # 0 -> 1 weight 1, 1 -> 0 weight 1, loop (1, 1) weight 3: the loop is replaced, not doubled
    ei = torch.tensor([[0, 1, 1], [1, 0, 1]])
    c = coef_of(*gcn_norm(ei, 2, torch.tensor([1.0, 1.0, 3.0])))
    assert len(c) == 4                                 # one loop per node
    # deg0 = 1 + 1 = 2, deg1 = 1 + 3 = 4
    assert c[(1, 1)] == pytest.approx(3 / 4) and c[(0, 0)] == pytest.approx(1 / 2)
    assert c[(0, 1)] == pytest.approx(1 / math.sqrt(8))
    # without weights the existing loop counts once, with weight 1
    c1 = coef_of(*gcn_norm(ei, 2))
    assert c1[(1, 1)] == pytest.approx(1 / 2) and c1[(0, 1)] == pytest.approx(1 / 2)


def test_gcn_norm_weighted_edges_and_isolated_node():
    # 0 <-> 1 weight 2, node 2 isolated: it keeps a loop of weight 1 and deg 1
    ei = torch.tensor([[0, 1], [1, 0]])
    c = coef_of(*gcn_norm(ei, 3, torch.tensor([2.0, 2.0])))
    assert c[(0, 1)] == pytest.approx(2 / 3) and c[(0, 0)] == pytest.approx(1 / 3)
    assert c[(2, 2)] == pytest.approx(1.0) and len(c) == 5


def test_gcn_norm_directed_uses_in_degree():
    # 0 -> 1, 0 -> 2, 1 -> 2 (flow source -> target): in-degrees with loops 1, 2, 3
    ei = torch.tensor([[0, 0, 1], [1, 2, 2]])
    c = coef_of(*gcn_norm(ei, 3))
    assert c[(0, 1)] == pytest.approx(1 / math.sqrt(2)) and c[(0, 2)] == pytest.approx(1 / math.sqrt(3))
    assert c[(1, 2)] == pytest.approx(1 / math.sqrt(6)) and (1, 0) not in c


def test_sort_pool_padding_and_tie_order():
    x = torch.tensor([[1.0, 0.5], [2.0, 0.5], [3.0, 0.9],          # graph 0: a tie at 0.5
                      [4.0, -0.0], [5.0, 0.0], [6.0, -1.0]], dtype=torch.float64)   # graph 1: -0 == +0
    out, index = sort_pool(x, [0, 3, 6], 4)
    assert index.tolist() == [[2, 0, 1, -1], [3, 4, 5, -1]]
    assert out.view(2, 4, 2)[0].tolist() == [[3.0, 0.9], [1.0, 0.5], [2.0, 0.5], [0.0, 0.0]]
    assert out.view(2, 4, 2)[1, 3].tolist() == [0.0, 0.0]
    out1, index1 = sort_pool(x, [0, 3, 6], 1)
    assert index1.tolist() == [[2], [3]] and out1.shape == (2, 2)


def test_sort_pool_all_negative_keys_and_n_equal_k():
    x = torch.tensor([[0.0, -3.0], [0.0, -1.0], [0.0, -2.0]], dtype=torch.float64)
    _, index = sort_pool(x, [0, 3], 3)
    assert index.tolist() == [[1, 2, 0]]


@pytest.mark.parametrize("counts,k,expect", [
    ([5, 8, 12, 20, 40], 0.6, 12),          # ceil(0.6 * 5) = 3 -> third smallest
    ([30, 10, 20, 50, 40], 0.6, 30),
    ([3, 4, 5, 6], 0.6, 10),                 # floor of 10
    ([100] * 7 + [200] * 3, 0.7, 100),       # ceil(7.0) = 7 -> the 7th
    ([100] * 7 + [200] * 3, 0.71, 200),
    ([15, 25], 1.0, 25),
    ([1, 2, 3], 35, 35),                     # k > 1 is a count
])
def test_sortpool_k_worked_examples(counts, k, expect):
    from s3grl_amd.seal_nn import sortpool_k

    assert sortpool_k(counts, k) == expect


def test_sortpool_k_dynamic_train_uses_first_1000():
    from s3grl_amd.seal_nn import sortpool_k

    counts = [50] * 1000 + [5] * 1000
    assert sortpool_k(counts, 0.6) == 50 and sortpool_k(counts, 0.5) == 10
    assert sortpool_k(counts, 0.5, dynamic_train=True) == 50
    assert sortpool_k(None, 0.6) == 30


def test_unused_arguments_raise_before_gpu_work():
    from s3grl_amd.seal_nn import DGCNNTwin, GCNTwin

    with pytest.raises(NotImplementedError):
        DGCNNTwin(32, 3, 1000, k=30, dropedge=0.2)
    with pytest.raises(NotImplementedError):
        DGCNNTwin(32, 3, 1000, k=30, node_embedding=torch.nn.Embedding(4, 2))
    with pytest.raises(NotImplementedError):
        GCNTwin(32, 3, 1000, dropedge=0.5)
    with pytest.raises(NotImplementedError):
        GCNTwin(32, 3, 1000, node_embedding=torch.nn.Embedding(4, 2))
    with pytest.raises(ValueError):
        DGCNNTwin(32, 3, 1000, k=30, use_feature=True)            # no features to size the first layer
    with pytest.raises(ValueError):
        DGCNNTwin(32, 3, 1000, k=9)                               # k = 9 leaves (int(4.5) - 4) * 32 = 0 MLP inputs
    with pytest.raises(NotImplementedError):
        from s3grl_amd.harness import train_and_evaluate_seal

        train_and_evaluate_seal((None, None), (None, None), model="SAGE")


def test_twin_shapes_and_state_dict_keys():
    from s3grl_amd.seal_nn import DGCNNTwin, GCNTwin

    m = DGCNNTwin(32, 3, 1000, k=30)
    sd = m.state_dict()
    assert sd["convs.0.lin.weight"].shape == (32, 32) and sd["convs.3.lin.weight"].shape == (1, 32)
    assert sd["convs.3.bias"].shape == (1,) and "convs.0.lin.bias" not in sd
    assert sd["conv1.weight"].shape == (16, 1, 97) and sd["conv2.weight"].shape == (32, 16, 5)
    assert sd["mlp.lins.0.weight"].shape == (128, (int((30 - 2) / 2 + 1) - 4) * 32)
    assert sd["mlp.norms.0.running_mean"].shape == (128,) and sd["mlp.lins.1.weight"].shape == (1, 128)
    g = GCNTwin(32, 3, 1000)
    assert [k for k in g.state_dict() if k.startswith("convs.")] == [
        "convs.0.bias", "convs.0.lin.weight", "convs.1.bias", "convs.1.lin.weight", "convs.2.bias",
        "convs.2.lin.weight"]
    assert g.state_dict()["mlp.lins.0.weight"].shape == (32, 32)


def test_ops_refuse_cpu_tensors():
    from s3grl_amd.seal_nn import sort_pool as hip_sort_pool

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_sort_pool(torch.zeros(3, 2), torch.tensor([0, 3]), 2)
