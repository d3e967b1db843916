"""CPU checks of node2vec pretraining: the fp64 restatement (tests/node2vec_reference.py) against torch's own autograd
on nn.Embedding(sparse=True) and torch.optim.SparseAdam, hand-computed answers at D = 2, window slicing, and the
argument checks of s3grl_amd.node2vec that refuse before any GPU work."""
import math

import numpy as np
import pytest
import torch

from node2vec_reference import loss_and_grad, sparse_adam, step, windows_of


def torch_steps(h0, batches, lr=0.01):
    """The reference's structure in float64: Node2Vec.loss on an nn.Embedding(sparse=True), SparseAdam."""
    emb = torch.nn.Embedding(h0.shape[0], h0.shape[1], sparse=True).double()
    with torch.no_grad():
        emb.weight.copy_(torch.as_tensor(h0))
    opt = torch.optim.SparseAdam(list(emb.parameters()), lr=lr)
    losses = []
    for pos, neg in batches:
        opt.zero_grad()
        loss = 0
        for rw, sign in ((torch.as_tensor(pos), 1), (torch.as_tensor(neg), -1)):
            start, rest = rw[:, 0], rw[:, 1:].contiguous()
            hs = emb(start).view(rw.size(0), 1, -1)
            hr = emb(rest.view(-1)).view(rw.size(0), -1, hs.shape[-1])
            out = (hs * hr).sum(dim=-1).view(-1)
            s = torch.sigmoid(out)
            loss = loss + (-torch.log((s if sign > 0 else 1 - s) + 1e-15).mean())
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    st = opt.state[emb.weight]
    return emb.weight.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy(), losses


def test_restatement_matches_torch_sparse_adam():
    rng = np.random.default_rng(0)
    n, d, C = 7, 5, 4
    h0 = rng.standard_normal((n, d))
    batches = []
    for b in range(4):
        pos = rng.integers(0, n, size=(6, C))
        pos[0, 1] = pos[0, 0]                       # a repeated row inside a window
        neg = rng.integers(0, n, size=(3 if b == 3 else 6, C))   # a short last batch
        if b == 1:
            pos[2] = 3                              # a window that is all one node
        batches.append((pos, neg))
    hw, mw, vw, lw = torch_steps(h0, batches)
    h, m, v = h0.copy(), np.zeros_like(h0), np.zeros_like(h0)
    for k, (pos, neg) in enumerate(batches):
        h, m, v, loss = step(h, m, v, k, pos, neg)
        assert loss == pytest.approx(lw[k], rel=1e-12)
    np.testing.assert_allclose(h, hw, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(m, mw, rtol=1e-12, atol=1e-16)
    np.testing.assert_allclose(v, vw, rtol=1e-12, atol=1e-20)


def test_untouched_rows_keep_state():
    h0 = np.arange(8.0).reshape(4, 2) / 10
    h, m, v, _ = step(h0, np.zeros_like(h0), np.zeros_like(h0), 0, [[0, 1]], [[0, 2]])
    assert np.array_equal(h[3], h0[3]) and not m[3].any() and not v[3].any()
    assert not np.array_equal(h[1], h0[1])


def test_hand_computed_d2():
    # h0 = (1, 0), h1 = (0.5, 1): one positive window (0, 1), one negative window (1, 0); out = 0.5 both
    h0 = np.array([[1.0, 0.0], [0.5, 1.0]])
    s = 1 / (1 + math.exp(-0.5))
    loss, grad, rows = loss_and_grad(h0, [[0, 1]], [[1, 0]])
    assert loss == pytest.approx(-math.log(s + 1e-15) - math.log(1 - s + 1e-15), rel=1e-14)
    gp = -s * (1 - s) / (s + 1e-15)                 # d(pos loss)/d out
    gn = s * (1 - s) / (1 - s + 1e-15)              # d(neg loss)/d out
    # node 0: pos start (gp · h1) + neg context (gn · h1);  node 1: pos context (gp · h0) + neg start (gn · h0)
    np.testing.assert_allclose(grad[0], (gp + gn) * h0[1], rtol=1e-14)
    np.testing.assert_allclose(grad[1], (gp + gn) * h0[0], rtol=1e-14)
    assert list(rows) == [0, 1]
    # first SparseAdam step: m = 0.1 g, v = 0.001 g², step_size = lr · sqrt(0.001) / 0.1  ->  h -= lr · g/(|g| + eps')
    h, m, v = sparse_adam(h0, np.zeros_like(h0), np.zeros_like(h0), 1, grad, rows, 0.01)
    np.testing.assert_allclose(m, 0.1 * grad, rtol=1e-14)
    np.testing.assert_allclose(v, 0.001 * grad ** 2, rtol=1e-12)
    expect = h0 - 0.01 * math.sqrt(0.001) / 0.1 * (0.1 * grad) / (np.sqrt(0.001) * np.abs(grad) + 1e-8)
    np.testing.assert_allclose(h, expect, rtol=1e-14)
    assert h[0, 1] == pytest.approx(-0.01, rel=1e-5)   # a unit step of lr against the gradient's sign


def test_window_slicing():
    rw = np.arange(2 * 6).reshape(2, 6)           # walk_length 5
    w = windows_of(rw, 5)                          # walk_length == context_size: 2 windows per row
    assert w.tolist() == [[0, 1, 2, 3, 4], [6, 7, 8, 9, 10], [1, 2, 3, 4, 5], [7, 8, 9, 10, 11]]
    assert windows_of(np.zeros((3, 21)), 10).shape == (36, 10)   # the paper's 12 windows per walk


def test_argument_checks_refuse_before_gpu(monkeypatch):
    from s3grl_amd import engine, node2vec
    from s3grl_amd.node2vec import Node2Vec

    def no_gpu(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(engine, "default_engine", no_gpu)
    ei = np.array([[0, 1], [1, 0]])
    with pytest.raises(NotImplementedError):
        Node2Vec(ei, 2, 4, p=2)
    with pytest.raises(NotImplementedError):
        Node2Vec(ei, 2, 4, q=0.5)
    with pytest.raises(NotImplementedError):
        Node2Vec(ei, 2, 4, sparse=False)
    with pytest.raises(ValueError):
        Node2Vec(ei, 2, 0)
    with pytest.raises(ValueError):
        Node2Vec(ei, 2, node2vec.MAX_DIM + 1)
    with pytest.raises(ValueError):
        Node2Vec(ei, 2, 4, walk_length=5, context_size=6)
    with pytest.raises(ValueError):
        Node2Vec(ei, 2, 4, context_size=1)
    with pytest.raises(ValueError):
        Node2Vec(ei, 2, 4, walks_per_node=0)
    with pytest.raises(ValueError):
        Node2Vec(ei, 0, 4)
    with pytest.raises(ValueError):
        Node2Vec(np.array([[0, 2], [1, 0]]), 2, 4)          # a node outside [0, N)
    with pytest.raises(ValueError):
        Node2Vec(np.array([0, 1, 1, 0]), 2, 4)              # not [2, E]
    with pytest.raises(ValueError):
        Node2Vec(ei, 2, 4, init=torch.zeros(3, 4))
    with pytest.raises(NotImplementedError):
        Node2Vec.fit(object.__new__(Node2Vec), 1, optimizer="Adam")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        node2vec.node_2_vec_pretrain("x", ei, 2, 4, 0, torch.device("cpu"), 1)


def test_csr_keeps_edge_index_as_given():
    from s3grl_amd.node2vec import csr_of

    # directed, a duplicate, a node without out-entries (3): rows are sources, order kept inside a row
    ip, ix = csr_of(np.array([[2, 0, 0, 2, 0], [1, 2, 1, 3, 1]]), 4)
    assert ip.tolist() == [0, 3, 3, 5, 5]
    assert ix.tolist() == [2, 1, 1, 1, 3]


def test_cache_file_is_read_without_gpu(tmp_path, monkeypatch):
    from s3grl_amd.node2vec import node_2_vec_pretrain

    monkeypatch.chdir(tmp_path)
    (tmp_path / "Emb").mkdir()
    x = torch.arange(6, dtype=torch.float32).view(3, 2)
    torch.save(x, tmp_path / "Emb" / "usair_2_seed1_k.pt")
    got = node_2_vec_pretrain("usair", np.zeros((2, 0)), 3, 2, 1, "cpu", 50, extra_identifier="k", cache=True)
    assert torch.equal(got, x)


# ---- what tests/test_gpu_node2vec_shapes.py rests on -----------------------------------------------------------------
def test_the_dimension_list_covers_every_lane_layout():
    """The D table of the GPU shape tests reaches all 14 (VEC, LPD) instantiations of dots_kernel, row_grad_kernel and
    adam_kernel, a second trip of the channel loop with and without float4, and groups whose last lanes own no
    channel."""
    from node2vec_checks import DIMS, lanes_rule

    assert {D: lanes_rule(D) for D in DIMS} == DIMS
    pairs = {(v, l) for v, l, _ in DIMS.values()}
    assert pairs == {(v, l) for v in (1, 4) for l in (1, 2, 4, 8, 16, 32, 64)} and len(pairs) == 14
    assert {v for v, l, t in DIMS.values() if t > 1} == {1, 4}            # a second trip with and without float4
    ragged = [D for D, (v, l, t) in DIMS.items() if D % (l * v)]
    assert sorted(ragged) == [3, 5, 12, 13, 17, 20, 33, 65, 260, 1000, 1028]
    assert any(DIMS[D][0] == 4 for D in ragged) and any(DIMS[D][0] == 1 for D in ragged)
    assert any(DIMS[D][2] > 1 for D in ragged)
    assert lanes_rule(20) == (4, 8, 1)                                    # 5 float4 columns on 8 lanes: 3 idle


@pytest.mark.parametrize("D", [3, 20, 65, 260])
def test_the_step_bound_sees_a_subtly_wrong_kernel(D):
    """The restatement mutated the way a wrong lane layout would compute, against `tolerances`: (a) one term of the
    hub row's gradient dropped, (b) the last channel never reached, (c) one of row_grad_kernel's S = 64 / LPD slices
    dropped from the hub row (every S-th term in key order; the whole row where S = 1).  Three steps, the second and
    third from non-zero moments.  Each must put exp_avg or exp_avg_sq past the bound at every step; the weight alone
    need not (from zero moments the first update is lr · sign(g), whatever |g| is)."""
    from node2vec_checks import (DIMS, HUB_BS, HUB_CFG, hub_graph, host_windows, init_table, row_terms, row_uses,
                                 tolerances)

    ei, n = hub_graph()
    S = 64 // DIMS[D][1]
    rng = np.random.default_rng(D)
    h = init_table(n, D, seed=D).double().numpy()
    m, v = np.zeros_like(h), np.zeros_like(h)
    perm = rng.permutation(n)
    for t in range(3):
        pos, neg = host_windows(ei, n, perm[t * HUB_BS:(t + 1) * HUB_BS], rng, **HUB_CFG)
        assert 64 < row_uses(pos, neg, 0) <= 4400
        _, grad, rows = loss_and_grad(h, pos, neg, fp32_sigmoid=True)
        terms = row_terms(h, pos, neg, 0)
        assert len(terms) == row_uses(pos, neg, 0)
        np.testing.assert_allclose(terms.sum(0), grad[0], rtol=1e-11, atol=1e-18)   # the terms are the row's gradient
        tm, tv, th = tolerances(h, m, v, t, pos, neg, 0.01)
        hr, mr, vr = sparse_adam(h, m, v, t + 1, grad, rows, 0.01)
        wrong = {"a": grad.copy(), "b": grad.copy(), "c": grad.copy()}
        wrong["a"][0] -= terms[len(terms) // 2]
        wrong["b"][:, D - 1] = 0
        wrong["c"][0] -= terms[S - 1::S].sum(0)
        for name, g in wrong.items():
            hw, mw, vw = sparse_adam(h, m, v, t + 1, g, rows, 0.01)
            rh, rm, rv = (float((np.abs(x - y) / tol).max()) for x, y, tol in ((hw, hr, th), (mw, mr, tm), (vw, vr, tv)))
            print(f"D={D} step {t} mutation ({name}): error / bound h {rh:.3g} m {rm:.3g} v {rv:.3g}")
            assert max(rm, rv) > 1, (name, t, rh, rm, rv)
        h, m, v = hr, mr, vr
