"""The SEAL models' HIP operators and twins on the MI355X: s3grl_amd.seal_nn against the fp64 restatement
(tests/seal_nn_reference.py), bit-identical repeats, and end-to-end training from enclosing_subgraphs output."""
import numpy as np
import pytest
import scipy.sparse as ssp
import torch

from conftest import GOLDEN, csr_from_arcs
from seal_nn_reference import dgcnn_forward, gcn_forward, gcn_norm, propagate, sort_order, sort_pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd.engine import Engine

    e = Engine("cuda:0")
    yield e
    e.close()


def _split(name, seed=0):
    from s3grl_amd import workloads as W

    n, e = W.load_topology(name)
    return W.edge_split(n, e, seed=seed)


def subgraphs(eng, li, A, hops, label, x=None, **kw):
    from s3grl_amd.seal import enclosing_subgraphs

    return enclosing_subgraphs(np.asarray(li), A, x, 0, hops, label, engine=eng, **kw)


@pytest.fixture(scope="module")
def usair(eng):
    sp = _split("usair")
    li, _ = sp.all_links()
    return sp.A, li, subgraphs(eng, li, sp.A, 2, "drnl")


def weighted(A, seed=3):
    U = ssp.triu(A, k=1).tocoo()
    w = np.random.default_rng(seed).integers(1, 5, size=U.nnz).astype(np.int64)
    W = ssp.coo_matrix((w, (U.row, U.col)), shape=A.shape)
    return (W + W.T).tocsr()


def check_propagation(subs, ids, H, use_edge_weight, seed=0):
    """Forward and backward of gcn_propagate on the batch `ids` against the restatement, on the device."""
    from s3grl_amd.seal_nn import gcn_propagate

    b = subs.batch(ids, use_edge_weight=use_edge_weight)
    g = torch.Generator(device="cuda").manual_seed(seed)
    h = torch.randn((b.num_nodes, H), device="cuda", generator=g).requires_grad_()
    bias = torch.randn(H, device="cuda", generator=g).requires_grad_()
    out = gcn_propagate(h, b, bias)
    gout = torch.randn_like(out)
    gh, gb = torch.autograd.grad(out, (h, bias), gout)
    src, dst, coef = gcn_norm(b.edge_index, b.num_nodes, b.edge_weight if use_edge_weight else None)
    ref = propagate(h.detach().double(), src, dst, coef) + bias.detach().double()
    ref_gh = propagate(gout.double(), dst, src, coef)
    torch.testing.assert_close(out.double(), ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gh.double(), ref_gh, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(gb, gout.sum(0))
    return b


@pytest.mark.parametrize("H", [1, 32, 37, 256])
def test_propagation_all_usair_links(usair, H):
    A, li, subs = usair
    L = len(subs)
    assert L == 7868
    ids = np.arange(L) if H <= 37 else np.arange(0, L, 4)
    b = check_propagation(subs, ids, H, False)
    assert b.num_nodes == (subs.subs.nodes.numel() if H <= 37 else int(subs.node_counts()[ids].sum()))


def test_propagation_shuffled_batch_and_edge_weights(eng, usair):
    A, li, _ = usair
    Aw = weighted(A)
    subs = subgraphs(eng, li[:, :1500], Aw, 2, "drnl")
    ids = np.random.default_rng(5).permutation(1500)[:300]
    for H in (1, 32):
        check_propagation(subs, ids, H, True)
        check_propagation(subs, ids, H, False)


def test_propagation_with_self_loops(eng, usair):
    A, li, _ = usair
    n = A.shape[0]
    rng = np.random.default_rng(7)
    loops = rng.choice(n, n // 3, replace=False)
    D = ssp.coo_matrix((rng.integers(2, 6, size=loops.size).astype(np.int64), (loops, loops)), shape=A.shape)
    Al = (weighted(A) + D).tocsr()
    subs = subgraphs(eng, li[:, :600], Al, 2, "drnl")
    s = subs.subs
    assert bool((s.src == s.dst).any())                    # the subgraphs carry (i, i) entries
    for use_w in (True, False):
        check_propagation(subs, np.arange(600), 32, use_w)
        check_propagation(subs, np.arange(600), 1, use_w)


def test_propagation_directed(eng):
    lab = np.load(GOLDEN / "labels_directed_usair.npz")
    A = csr_from_arcs(int(lab["num_nodes"]), lab["arcs"])
    subs = subgraphs(eng, lab["links"].T, A, 2, "drnl", directed=True)
    s = subs.subs
    first = np.repeat(subs._node_ptr[:-1], np.diff(subs._edge_ptr))
    arcs = set(zip((s.src.cpu().numpy() + first).tolist(), (s.dst.cpu().numpy() + first).tolist()))
    assert any((v, u) not in arcs for u, v in arcs)        # really directed
    for H in (1, 32, 37):
        check_propagation(subs, np.arange(len(subs)), H, False)


def pool_case(sizes, D, seed, keys=None):
    g = torch.Generator().manual_seed(seed)
    n = int(sum(sizes))
    x = torch.randn((n, D), generator=g)
    if keys is not None:
        x[:, -1] = keys(n, g)
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.as_tensor(sizes), 0)
    return x, ptr


def check_sort_pool(x, ptr, k, lds_budget=0):
    from s3grl_amd.seal_nn import sort_pool as hip_sort_pool

    xd = x.cuda().requires_grad_()
    out, index = hip_sort_pool(xd, ptr.cuda(), k, int(ptr.diff().max()), lds_budget, return_index=True)
    ref, ref_index = sort_pool(x.double(), ptr, k)
    assert torch.equal(index.cpu().long(), ref_index)
    assert torch.equal(out.cpu(), ref.float())
    gout = torch.randn_like(out)
    (gx,) = torch.autograd.grad(out, xd, gout)
    xr = x.double().requires_grad_()
    (ref_gx,) = torch.autograd.grad(sort_pool(xr, ptr, k)[0], xr, gout.cpu().double())
    assert torch.equal(gx.cpu(), ref_gx.float())
    return out, index, gx


@pytest.mark.parametrize("D", [97, 769])
def test_sort_pool_sizes_and_widths(eng, D):
    k = 12
    sizes = [3, 12, 40, 1, 12, 200, 11, 13]                 # n < k, n = k, n > k
    x, ptr = pool_case(sizes, D, 1)
    check_sort_pool(x, ptr, k)
    check_sort_pool(x, ptr, k, lds_budget=1)               # every graph through the HBM path
    check_sort_pool(x, ptr, 1)                             # k = 1
    check_sort_pool(*pool_case([57], D, 2), 30)            # B = 1


def test_sort_pool_ties_signed_zero_and_negative_keys(eng):
    ties = pool_case([30, 30, 5], 97, 3, keys=lambda n, g: torch.randint(0, 3, (n,), generator=g).float() * 0.5)
    check_sort_pool(*ties, 10)
    x, ptr = pool_case([6, 6], 97, 4)
    x[:, -1] = torch.tensor([-0.0, 0.0, -0.0, 1.0, 0.0, -1.0, -0.0, -0.0, 0.0, 0.0, -0.0, -2.0])
    _, index, _ = check_sort_pool(x, ptr, 6)
    assert index.cpu().tolist()[0] == [3, 0, 1, 2, 4, 5]
    neg = pool_case([25, 9], 769, 5, keys=lambda n, g: -torch.rand(n, generator=g) - 0.5)
    check_sort_pool(*neg, 16)


def test_sort_pool_star_beyond_65535_nodes(eng):
    """A 70 001-node graph sorts in HBM (its keys exceed the LDS budget); small graphs beside it stay on chip."""
    x, ptr = pool_case([70001, 20, 3], 97, 6)
    check_sort_pool(x, ptr, 300)


def test_determinism(usair):
    from s3grl_amd.seal_nn import gcn_propagate
    from s3grl_amd.seal_nn import sort_pool as hip_sort_pool

    _, _, subs = usair
    b = subs.batch(np.arange(2000))
    runs = []
    for _ in range(2):
        g = torch.Generator(device="cuda").manual_seed(11)
        h = torch.randn((b.num_nodes, 97), device="cuda", generator=g).requires_grad_()
        out = gcn_propagate(h, b)
        (gh,) = torch.autograd.grad(out, h, torch.ones_like(out))
        hp = h.detach().clone().requires_grad_()
        pooled = hip_sort_pool(hp, b.node_ptr, 150, b.max_nodes)
        (gp,) = torch.autograd.grad(pooled, hp, torch.ones_like(pooled) * 0.5)
        runs.append((out, gh, pooled, gp))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


def test_batch_matches_collate(eng):
    sp = _split("usair")
    li, _ = sp.all_links()
    x = torch.randn(sp.A.shape[0], 5, generator=torch.Generator().manual_seed(2))
    subs = subgraphs(eng, li[:, :700], sp.A, 2, "de", x=x)
    full, whole = subs.batch(np.arange(700)), subs.collate_pyg()
    for key in ("x", "z", "edge_index", "edge_weight"):
        assert torch.equal(getattr(full, key), getattr(whole, key)), key
    assert torch.equal(full.node_ptr, whole.ptr) and full.max_nodes == int(subs.node_counts().max())
    ids = np.array([650, 3, 77, 3, 0])
    part = subs.batch(ids)
    for j, i in enumerate(ids):
        d, a, b = subs[int(i)], int(part.node_ptr[j]), int(part.node_ptr[j + 1])
        assert torch.equal(part.x[a:b], d.x) and torch.equal(part.z[a:b], d.z)
    ei = part.edge_index
    assert torch.equal(ei[:, ei[0] >= int(part.node_ptr[4])] - int(part.node_ptr[4]), subs[0].edge_index)


def _twin_inputs(eng, label, n_links=48, F=6):
    sp = _split("usair")
    li, _ = sp.all_links()
    x = torch.randn(sp.A.shape[0], F, generator=torch.Generator().manual_seed(9))
    subs = subgraphs(eng, li[:, ::97][:, :n_links], sp.A, 2, label, x=x)
    b = subs.batch(np.arange(len(subs))[::-1].copy())
    assert torch.equal(b.x.cpu(), x[subs.subs.nodes[b.rows].long().cpu()])
    b.x = b.x.clone().requires_grad_()
    return subs, b


def _ref_inputs(b):
    return (b.z.cpu(), b.x.detach().cpu().double().requires_grad_(), b.edge_index.cpu(), None, b.node_ptr.cpu())


def test_dgcnn_twin_against_restatement(eng, monkeypatch):
    from s3grl_amd import seal_nn

    torch.manual_seed(0)
    subs, b = _twin_inputs(eng, "drnl")
    model = seal_nn.DGCNNTwin(32, 3, 1000, k=0.6, train_dataset=subs, use_feature=True).cuda().eval()
    seen = {}
    orig = seal_nn.sort_pool

    def spy(*a, **kw):
        out, index = orig(*a, return_index=True, **kw)
        seen["index"] = index
        return out

    monkeypatch.setattr(seal_nn, "sort_pool", spy)
    out = model(b)
    (gx,) = torch.autograd.grad(out.sum(), b.x)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    z, x, ei, ew, ptr = _ref_inputs(b)
    states = {}
    ref = dgcnn_forward(sd, z, x, ei, ew, ptr, k=model.k, num_convs=4, index=seen["index"].cpu(), states=states)
    (ref_gx,) = torch.autograd.grad(ref.sum(), x)
    # the twin's order is the restatement's wherever fp32 and fp64 keys cannot disagree
    key = states["h"][:, -1].detach()
    own = sort_order(states["h"].detach(), ptr, model.k)
    idx = seen["index"].cpu().long()
    for g in range(idx.shape[0]):
        mine, theirs = idx[g][idx[g] >= 0], own[g][own[g] >= 0]
        assert mine.numel() == theirs.numel()
        assert torch.all(key[mine][:-1] >= key[mine][1:] - 1e-5)
        assert torch.allclose(key[mine], key[theirs], atol=1e-5, rtol=0)
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gx.cpu().double(), ref_gx, rtol=1e-4, atol=1e-4)


def test_gcn_twin_against_restatement(eng):
    from s3grl_amd import seal_nn

    torch.manual_seed(0)
    subs, b = _twin_inputs(eng, "de")
    assert b.z.dim() == 2
    model = seal_nn.GCNTwin(32, 3, 1000, train_dataset=subs, use_feature=True).cuda().eval()
    out = model(b)
    (gx,) = torch.autograd.grad(out.sum(), b.x)
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    z, x, ei, ew, ptr = _ref_inputs(b)
    ref = gcn_forward(sd, z, x, ei, ew, ptr, num_convs=3)
    (ref_gx,) = torch.autograd.grad(ref.sum(), x)
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gx.cpu().double(), ref_gx, rtol=1e-4, atol=1e-4)


def usair_seal_splits(eng, label, seed):
    sp = _split("usair", seed=seed)

    def prep(name):
        pos, neg = sp.links[name]
        li = np.concatenate([pos, neg], axis=1)
        y = torch.cat([torch.ones(pos.shape[1]), torch.zeros(neg.shape[1])]).to(eng.device)
        return subgraphs(eng, li, sp.A, 2, label), y

    return prep("train"), prep("test")


# Thresholds: the lowest test AUC of seeds 1, 2, 3 measured on the MI355X (4 epochs at lr 1e-3), less a margin:
# DGCNN/drnl 0.9776, 0.9717, 0.9732 -> 0.95; GCN/de 0.9683, 0.9577, 0.9689 -> 0.93.
@pytest.mark.parametrize("model,label,epochs,threshold", [("DGCNN", "drnl", 4, 0.95), ("GCN", "de", 4, 0.93)])
def test_usair_end_to_end_auc(eng, model, label, epochs, threshold):
    from s3grl_amd.harness import train_and_evaluate_seal

    train, test = usair_seal_splits(eng, label, seed=1)
    auc, _ = train_and_evaluate_seal(train, test, model=model, hidden=32, num_layers=3, k=0.6, epochs=epochs,
                                     lr=1e-3, seed=1)
    print(f"[seal_nn] USAir 2-hop {model}/{label}, {epochs} epochs at lr 1e-3: test AUC {auc:.4f}")
    assert auc > threshold, auc
