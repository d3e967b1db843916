"""WalkPool without a GPU: hand-derived answers that pin the dense restatement (tests/walkpool_reference.py), the
argument checks of the two operators, the kernels' layout and the twin's parameter names."""
import math

import pytest
import torch

import walkpool_reference as R

TAUS = (2, 3, 4, 5)


def _features(n, edges, heads=1, hidden=4, dtype=torch.float64):
    """All logits 0 (q = k = 0): every arc into a node weighs the same."""
    src = torch.tensor([a for a, b in edges] + [b for a, b in edges], dtype=torch.long)
    dst = torch.tensor([b for a, b in edges] + [a for a, b in edges], dtype=torch.long)
    q = torch.zeros((n, heads, hidden), dtype=dtype)
    Pp, Pm, omega, _ = R.attention_dense(q, q, n, src, dst)
    walks, _ = R.walk_features(Pp, Pm, len(TAUS))
    return Pp, Pm, omega, walks


def test_isolated_pair_known_answer():
    Pp, Pm, omega, walks = _features(2, [])
    assert torch.equal(Pm, torch.zeros_like(Pm))
    assert omega.tolist() == [1.0]
    w = walks[0]
    assert w[:, 0].tolist() == [2, 0, 2, 0]        # graphlevel
    assert w[:, 1].tolist() == [2, 0, 2, 0]        # nodelevel_p
    assert w[:, 3].tolist() == [0, 2, 0, 2]        # linklevel_p
    assert w[:, 2].tolist() == [0, 0, 0, 0] and w[:, 4].tolist() == [0, 0, 0, 0]


def test_triangle_known_answer():
    _, _, omega, walks = _features(3, [(0, 2), (1, 2)])
    w = walks[0]
    assert omega.tolist() == [1.0]
    for t, tau in enumerate(TAUS):
        a = (-0.5) ** tau
        even = 1.0 if tau % 2 == 0 else 0.0
        assert w[t, 1].item() == pytest.approx(2 * (1 + 2 * a) / 3, abs=1e-14)
        assert w[t, 3].item() == pytest.approx(2 * (1 - a) / 3, abs=1e-14)
        assert w[t, 2].item() == pytest.approx(even, abs=1e-14)
        assert w[t, 4].item() == pytest.approx(even, abs=1e-14)
        assert w[t, 0].item() == pytest.approx((1 + 2 * a) - 2 * even, abs=1e-14)
    assert w[:, 0].tolist() == pytest.approx([-0.5, 0.75, -0.875, 0.9375], abs=1e-14)


def test_feature_row_order():
    heads, walk_len = 2, 3
    walks = torch.arange(heads * walk_len * 5, dtype=torch.float64).view(heads, walk_len, 5)
    omega = torch.tensor([-1.0, -2.0], dtype=torch.float64)
    row = R.feature_row(walks, omega)
    assert row.numel() == heads * (5 * walk_len + 1)
    assert row[:6].tolist() == [walks[h, t, 0].item() for h in range(2) for t in range(3)]
    assert row[6:8].tolist() == [-1.0, -2.0]
    assert row[8:14].tolist() == [walks[h, t, 1].item() for h in range(2) for t in range(3)]
    assert row[-6:].tolist() == [walks[h, t, 4].item() for h in range(2) for t in range(3)]


def test_only_in_arc_is_the_candidate():
    """Node 1 hangs on node 0 alone: without the candidate arc it has no in-arc, its weights_m and its row of P- are 0."""
    torch.manual_seed(0)
    n = 3                                                     # E- = {0 - 2}
    src = torch.tensor([0, 2]), torch.tensor([2, 0])
    q, k = torch.randn(n, 2, 4, dtype=torch.float64), torch.randn(n, 2, 4, dtype=torch.float64)
    Pp, Pm, _, _ = R.attention_dense(q, k, n, src[0], src[1])
    assert torch.equal(Pm[:, 1, :], torch.zeros(2, n, dtype=torch.float64))
    assert torch.equal(Pp[:, 1, :], torch.tensor([[1.0, 0, 0]] * 2, dtype=torch.float64))
    assert torch.allclose(Pp.sum(-1), torch.ones(2, n, dtype=torch.float64))
    assert torch.allclose(Pm[:, [0, 2]].sum(-1), torch.ones(2, 2, dtype=torch.float64))


class _FakeBatch:
    num_nodes, num_arcs, num_graphs, max_nodes = 4, 6, 1, 4


def test_attention_argument_checks():
    from s3grl_amd import walkpool as wp

    q = torch.zeros(4, 2, 8)
    with pytest.raises(ValueError, match="float32"):
        wp.attention_weights(q.double(), q.double(), _FakeBatch())
    with pytest.raises(ValueError, match="float32"):
        wp.attention_weights(q[0], q[0], _FakeBatch())
    with pytest.raises(ValueError, match="differ in shape"):
        wp.attention_weights(q, q[:, :1], _FakeBatch())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wp.attention_weights(q, q, _FakeBatch())


def test_walk_pool_argument_checks():
    from s3grl_amd import walkpool as wp

    w = torch.zeros(6, 2)
    for bad in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match="walk_len"):
            wp.walk_pool(w, w, _FakeBatch(), bad)
    with pytest.raises(ValueError, match="float32"):
        wp.walk_pool(w.double(), w.double(), _FakeBatch(), 3)
    with pytest.raises(ValueError, match="float32"):
        wp.walk_pool(w[0], w[0], _FakeBatch(), 3)
    with pytest.raises(ValueError, match="differ in shape"):
        wp.walk_pool(w, w[:3], _FakeBatch(), 3)
    with pytest.raises(ValueError, match="lds_budget"):
        wp.walk_pool(w, w, _FakeBatch(), 3, lds_budget=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wp.walk_pool(w, w, _FakeBatch(), 3)
    with pytest.raises(ValueError, match="walk_len"):
        wp.WalkPooling(8, 8, walk_len=17)


def test_run_walkpool_refuses_directed_graphs():
    import numpy as np
    import scipy.sparse as ssp

    from s3grl_amd import walkpool as wp
    from s3grl_amd.workloads import Split

    A = ssp.csr_matrix((np.ones(2), ([0, 1], [1, 2])), shape=(3, 3))        # 0 -> 1 -> 2, one direction each
    with pytest.raises(NotImplementedError, match="directed"):
        wp.run_walkpool(Split(3, np.array([[0, 1], [1, 2]]), A, {}))


def test_layout_values():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd import walkpool as wp

    # the default budget is 80 KiB: forward holds 2 arrays of n x W floats, backward walk_len + 2
    lay = wp.layout(300, 5000, 2, 7)
    assert lay["forward"] == {"block": 32, "groups": 8, "flavour": "lds",
                              "workspace_bytes": 4 * 2 * 2 * 8 * 7}
    assert lay["backward"]["block"] == 4 and lay["backward"]["flavour"] == "lds"    # 9·300·8·4 > 80 KiB >= 9·300·4·4
    assert lay["backward"]["workspace_bytes"] == 4 * 8 * 2 * 5000 * 2
    # the block stays below 2 n; a pair is one block of 4
    assert wp.layout(2, 2, 1, 1)["forward"] == {"block": 4, "groups": 1, "flavour": "lds", "workspace_bytes": 8}
    assert wp.layout(10, 40, 1, 2)["forward"]["block"] == 16
    assert wp.layout(10, 40, 1, 2)["forward"]["groups"] == 1
    # a budget that forces several blocks per link
    small = wp.layout(40, 200, 1, 2, lds_budget=2 * 40 * 4 * 4)
    assert small["forward"]["block"] == 4 and small["forward"]["groups"] == 8 and small["forward"]["flavour"] == "lds"
    assert small["backward"]["flavour"] == "hbm"                                    # 4 arrays do not fit 2 arrays' budget
    # everything through HBM
    hbm = wp.layout(300, 5000, 2, 7, lds_budget=1)
    assert hbm["forward"]["flavour"] == "hbm" and hbm["forward"]["block"] == 4
    assert hbm["forward"]["workspace_bytes"] == 4 * 2 * 2 * 8 * (7 + 2 * 300 * 4)
    assert hbm["backward"]["workspace_bytes"] == 4 * (2 * 2 * 8 * 9 * 300 * 4 + 8 * 2 * 5000 * 2)
    # 4096 nodes: W = 4 needs 128 KiB, above the default budget; it fits the largest one
    assert wp.layout(4096, 10, 1, 7)["forward"]["flavour"] == "hbm"
    assert wp.layout(4096, 10, 1, 7, lds_budget=159 << 10)["forward"] == {
        "block": 4, "groups": 8, "flavour": "lds", "workspace_bytes": 4 * 2 * 8 * 7}
    with pytest.raises(NotImplementedError):
        wp.layout(4097, 10, 1, 7)
    with pytest.raises(ValueError):
        wp.layout(10, 10, 1, 17)
    with pytest.raises(ValueError):
        wp.layout(10, 10, 0, 3)


def test_state_dict_names_and_shapes():
    from s3grl_amd.walkpool import LinkPredTwin

    heads, walk_len, hid, F_in = 2, 7, 32, 16
    m = LinkPredTwin(F_in + hid, hid, heads, walk_len, drnl=True, z_max=50)
    sd = m.state_dict()
    L = heads * (5 * walk_len + 1)
    expect = {"z_embedding.weight": (50, hid), "conv1.lin.weight": (hid, F_in + hid), "conv1.bias": (hid,),
              "conv2.lin.weight": (hid, hid), "conv2.bias": (hid,),
              "wp.lin_key1.weight": (hid, F_in + 3 * hid), "wp.lin_query1.weight": (hid, F_in + 3 * hid),
              "wp.lin_key2.weight": (heads * hid, hid), "wp.lin_query2.weight": (heads * hid, hid),
              "classifier.nn.weight": (L,), "classifier.linear1.weight": (20 * L, L),
              "classifier.linear2.weight": (20 * L, 20 * L), "classifier.linear3.weight": (10 * L, 20 * L),
              "classifier.linear4.weight": (L, 10 * L), "classifier.linear5.weight": (1, L)}
    for name, shape in expect.items():
        assert tuple(sd[name].shape) == shape, name
    ref = R.DenseLinkPred(F_in + hid, hid, heads, walk_len, drnl=True, z_max=50)
    assert set(ref.state_dict()) == set(sd)
    ref.load_state_dict(sd)
    assert "z_embedding.weight" not in LinkPredTwin(8, 8).state_dict()
    assert math.prod(sd["classifier.linear5.weight"].shape) == L


def test_package_exports():
    import s3grl_amd

    for name in ("run_walkpool", "WalkPoolSplit", "LinkPredTwin"):
        assert callable(getattr(s3grl_amd, name))
