"""node2vec pretraining on the MI355X (s3grl_amd.node2vec, csrc/s3grl_node2vec.hip): the windows the engine draws
against PyG's sampling contract, teacher-forced step parity with the fp64 restatement (tests/node2vec_reference.py),
the step hook against the engine's own steps, determinism, edge cases, embedding quality and the paper's USAir
PoS Plus entry end to end."""
import numpy as np
import pytest
import torch

from node2vec_checks import check_windows as _check_windows
from node2vec_checks import parity as _parity
from node2vec_checks import same_state as _same_state

pytestmark = pytest.mark.gpu


def _usair_train():
    from s3grl_amd import workloads as W

    n, e = W.load_topology("usair")
    return W.edge_split(n, e, seed=0)


def _sink_graph():
    """40 nodes, directed arcs: node 39 has no edges at all, node 38 only in-arcs (a sink)."""
    rng = np.random.default_rng(5)
    src = rng.integers(0, 38, 150)
    dst = rng.integers(0, 39, 150)
    return np.stack([src, dst]), 40


def test_windows_follow_pyg_sampling():
    from s3grl_amd.node2vec import Node2Vec

    sp = _usair_train()
    n2v = Node2Vec(sp.edge_index(), sp.num_nodes, 16, seed=3)
    p0 = _check_windows(n2v, sp.edge_index(), sp.num_nodes, 0)
    p1 = _check_windows(n2v, sp.edge_index(), sp.num_nodes, 7)
    assert not np.array_equal(p0, p1)
    ei, N = _sink_graph()
    g = Node2Vec(ei, N, 4, walk_length=6, context_size=3, walks_per_node=3, num_negative_samples=2, seed=1)
    for e in (0, 2):
        _check_windows(g, ei, N, e, bs=7)
    pos, _ = g.windows(0, 0, 7)
    pos = pos.cpu().numpy()
    # the isolated node and the sink stay where they are once reached
    assert np.all(pos[pos[:, 0] == 39] == 39)


def test_star_neighbour_choice_is_uniform():
    from s3grl_amd.node2vec import Node2Vec

    k = 12                                                         # centre 0, leaves 1..12, both directions
    ei = np.array([[0] * k + list(range(1, k + 1)), list(range(1, k + 1)) + [0] * k])
    n2v = Node2Vec(ei, k + 1, 4, walk_length=20, context_size=2, seed=11)
    counts = np.zeros(k + 1)
    for e in range(20):
        pos, _ = n2v.windows(e, 0, 32)
        pos = pos.cpu().numpy()
        nxt = pos[pos[:, 0] == 0, 1]
        counts += np.bincount(nxt, minlength=k + 1)
    assert counts[0] == 0
    obs = counts[1:]
    exp = obs.sum() / k
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    assert obs.sum() > 10000 and chi2 < 40.0, (obs, chi2)         # 11 dof: P(chi2 > 40) < 1e-4


def test_step_parity_teacher_forced_d16():
    from s3grl_amd.node2vec import Node2Vec

    sp = _usair_train()
    n2v = Node2Vec(sp.edge_index(), sp.num_nodes, 16, seed=0)
    worst = _parity(n2v, 220)
    print("[n2v] D=16 parity, worst |err| / tol for h, m, v, loss rel:", worst)


def test_step_parity_teacher_forced_d256():
    from s3grl_amd.node2vec import Node2Vec

    sp = _usair_train()
    n2v = Node2Vec(sp.edge_index(), sp.num_nodes, 256, seed=0)
    worst = _parity(n2v, 6)
    print("[n2v] D=256 parity, worst |err| / tol for h, m, v, loss rel:", worst)


def test_step_hook_equals_engine_draw():
    from s3grl_amd.node2vec import Node2Vec

    sp = _usair_train()
    a = Node2Vec(sp.edge_index(), sp.num_nodes, 16, seed=4)
    b = Node2Vec(sp.edge_index(), sp.num_nodes, 16, seed=4)
    la = a.fit(2)
    lb = []
    for e in range(2):
        lb.append(sum(b.step(*b.windows(e, s)) for s in range(b.steps_per_epoch())))
    assert _same_state(a, b)
    np.testing.assert_allclose(la, lb, rtol=1e-6)   # per-step losses are identical; the host sums in another order


def test_fit_is_deterministic():
    from s3grl_amd.node2vec import Node2Vec

    sp = _usair_train()
    runs = [Node2Vec(sp.edge_index(), sp.num_nodes, 16, seed=s) for s in (9, 9, 10)]
    losses = [r.fit(3) for r in runs]
    assert _same_state(runs[0], runs[1]) and losses[0] == losses[1]
    assert not torch.equal(runs[0].embedding(), runs[2].embedding())


@pytest.mark.parametrize("N,dim,neg", [(10, 8, 1), (45, 1, 2), (70, 3, 1)])
def test_edge_cases(N, dim, neg):
    """N < 32 (one short batch), N % 32 != 0, isolated nodes, two negatives per walk, D = 1 and D = 3 (scalar lanes)."""
    from s3grl_amd.node2vec import Node2Vec

    rng = np.random.default_rng(N)
    e = rng.integers(0, N - 2, size=(2, 3 * N))                      # nodes N-2, N-1: no edges
    n2v = Node2Vec(e, N, dim, walk_length=8, context_size=4, num_negative_samples=neg, seed=2)
    _check_windows(n2v, e, N, 0, bs=32)
    _parity(n2v, 4)
    losses = n2v.fit(2)
    assert len(losses) == 2 and all(np.isfinite(losses))
    assert torch.isfinite(n2v.embedding()).all()


def _dot_auc(seed):
    from s3grl_amd.harness import auc_score
    from s3grl_amd.node2vec import Node2Vec

    sp = _usair_train()
    n2v = Node2Vec(sp.edge_index(), sp.num_nodes, 16, seed=seed)
    n2v.fit(50)
    h = n2v.embedding()
    pos, neg = (torch.as_tensor(x).to(h.device) for x in sp.links["test"])
    score = torch.cat([(h[pos[0]] * h[pos[1]]).sum(1), (h[neg[0]] * h[neg[1]]).sum(1)])
    y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(h.device)
    return auc_score(score, y)


def test_embedding_quality_usair():
    """Dot-product AUC of USAir's test positives against its test negatives after the paper's 50 epochs (D = 16).
    Measured with node2vec seeds 0, 1, 2 (tools/n2v_probe.py, profiles/n2v_probe.json): 0.9069, 0.9224, 0.9113;
    the threshold leaves a margin of about 0.03 below the lowest."""
    auc = _dot_auc(0)
    print("[n2v] USAir dot-product test AUC, seed 0:", auc)
    assert auc > THRESHOLD_QUALITY, auc


def test_usair_posplus_n2v_end_to_end():
    """configs/paper/auc_s3grl.json's USAir PoS Plus entry: node2vec features (dim 16, 50 epochs), sign_k 3, 2 hops,
    k_heuristic 1, mean pool, on the engine's operators and the SIGNNet twin.  Measured with the workload's node2vec
    seed 0 and training seeds 1, 2, 3 (tools/n2v_probe.py, profiles/n2v_probe.json): 0.9611, 0.9589, 0.9611; the
    threshold leaves a margin of about 0.03 below the lowest."""
    from s3grl_amd import workloads
    from s3grl_amd.engine import Engine
    from s3grl_amd.harness import train_and_evaluate

    w = workloads.make("usair_posplus_k3_n2v")
    assert w.X.shape == (w.split.num_nodes, 16)
    np.testing.assert_allclose(w.X.sum(1)[w.X.sum(1) >= 1], 1, rtol=1e-5)
    eng = Engine("cuda:0")
    G, f = eng.graph(w.A), eng.features(w.X)

    def prep(split):
        pos, neg = w.split.links[split]
        li = np.concatenate([pos, neg], axis=1)
        y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
        res = eng.precompute(G, f, eng.links(li), mode=w.mode, num_hops=w.num_hops, sign_k=w.sign_k)
        return res.rows, res.row_ptr, y

    auc, _ = train_and_evaluate(prep("train"), prep("test"), k_heuristic=1, k_pool_strategy="mean", epochs=8,
                                lr=2e-3, seed=1)
    print("[n2v] usair_posplus_k3_n2v test AUC:", auc)
    eng.close()
    assert auc > THRESHOLD_E2E, auc


THRESHOLD_QUALITY = 0.88
THRESHOLD_E2E = 0.93
