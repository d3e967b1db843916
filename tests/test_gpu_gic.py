"""Graph InfoClust on the GPU: `GicGraph`, the soft k-means and cluster-discriminator kernels (s3grl_gic_*), the twin's
teacher-forced step against the reference-pinned golden files, a layout sweep against the restatement, determinism,
the loop's step rule and the USAir row end to end.  Every comparison is a relative Frobenius error held to
`gic_reference.bound` (8 x the reference's own fp32-vs-fp64 error of that quantity + the floor of one fp32 sum); each
test prints error, bound and the reference's fp32 error."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))

import gic_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _gic():
    from s3grl_amd import gic

    return gic


@functools.lru_cache(maxsize=None)
def _case(case):
    """(golden, restatement fp64 outputs, restatement fp32 outputs), computed once per case and never modified."""
    g, o64 = R.restated(case)
    _, o32 = R.restated(case, torch.float32)
    return g, o64, o32


def _size(g):
    return int(g["num_nodes"]) + int(g["dim"]) + int(g["K"])


def _hold(name, got, want, ref32, n):
    err, ref, lim = R.rel(got, want), R.rel(ref32, want), R.bound(ref32, want, n)
    print(f"{name}: err {err:.3e}  reference fp32 {ref:.3e}  bound {lim:.3e}  err/bound {err / lim:.3f}")
    assert err <= lim, (name, err, lim)


def _hold_golden(g, key, got, n):
    """`got` (a whole array) against the golden fp64 rows of `key`, bounded by the golden fp32 copy's error."""
    _hold(key, R.stored(g, key, got.detach().cpu()), g[key], g["f32_" + key], n)


# ---- operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny", "rand300", "usair"])
def test_propagate_against_golden_operator(case):
    from s3grl_amd.propagate import GicGraph

    g = R.golden(case)
    n = int(g["num_nodes"])
    M = R.dense((g["op_row"], g["op_col"], g["op_val"]), n)
    gen = torch.Generator().manual_seed(5)
    h = torch.randn((n, 7), generator=gen)
    w = torch.randn((n, 7), generator=gen)
    bias = torch.randn(7, generator=gen)
    graph = GicGraph(g["arcs"].T, n, DEV)
    hd = h.to(DEV).requires_grad_(True)
    bd = bias.to(DEV).requires_grad_(True)
    out = graph.propagate(hd, bd)
    (out * w.to(DEV)).sum().backward()
    M32 = M.float()
    _hold("propagate", out, M @ h.double() + bias.double(), M32 @ h + bias, n)
    _hold("propagate grad", hd.grad, M.T @ w.double(), M32.T @ w, n)
    _hold("propagate bias grad", bd.grad, w.double().sum(0), w.sum(0), n)


# ---- kernels against the golden files ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES)
def test_clusterator_forward(case):
    gic = _gic()
    g, o64, o32 = _case(case)
    n, beta = _size(g), float(g["beta"])
    h1 = o64["h1"].float().to(DEV)
    init = torch.as_tensor(g["p_init"]).float().to(DEV)
    mu10, _ = gic.cluster(h1, init, beta, 10)
    Z, S = gic.clusterator(h1, init, beta)
    for key, got in (("mu10", mu10), ("Z", Z), ("S", S)):
        _hold_golden(g, key, got, n)
        _hold(key + " (whole)", got, o64[key], o32[key], n)
    _, r1 = gic.cluster(h1, mu10, beta, 1)
    assert torch.equal(r1, S)


def _leaf(t):
    """t itself as an autograd leaf: the same storage, strides and address, no copy."""
    return t.detach().requires_grad_(True)


def _watch(layout, **tensors):
    """Asserts that the tensors handed to s3grl_amd.gic have the layout under test; on a non-leaf, that the gradient
    autograd hands to its backward has it too."""
    if layout is None:
        return
    for name, t in tensors.items():
        if t.is_leaf:
            layout(name, t)
        else:
            t.register_hook(lambda g, name=name: layout("grad of " + name, g))


def _kernel_pass(fn_cluster, fn_disc, h1, h2, init, beta, w, layout=None):
    """Z, S, logits2 and the gradients of w · logits2 with respect to h1 and h2; w is the upstream gradient itself."""
    h1, h2 = _leaf(h1), _leaf(h2)
    _watch(layout, h1=h1, h2=h2, init=init, w=w)
    Z, S = fn_cluster(h1, init, beta)[:2]
    logits2 = fn_disc(S, Z, h1, h2)
    _watch(layout, logits2=logits2)
    logits2.backward(w)
    return {"Z": Z, "S": S, "logits2": logits2, "g_h1": h1.grad, "g_h2": h2.grad}


def _cluster_pass(fn_cluster, h1, init, beta, gZ, gS, layout=None):
    """The gradient with respect to h1 of the Clusterator alone, from given upstream gradients of Z and S."""
    h1 = _leaf(h1)
    _watch(layout, h1=h1, init=init, gZ=gZ, gS=gS)
    Z, S = fn_cluster(h1, init, beta)[:2]
    _watch(layout, Z=Z, S=S)
    torch.autograd.backward([Z, S], [gZ, gS])
    return {"g_h1": h1.grad}


def _disc_pass(fn_disc, S, Z, h1, h2, w, layout=None):
    leaves = [_leaf(t) for t in (S, Z, h1, h2)]
    _watch(layout, S=leaves[0], Z=leaves[1], h1=leaves[2], h2=leaves[3], w=w)
    out = fn_disc(*leaves)
    _watch(layout, logits2=out)
    out.backward(w)
    return {"logits2": out, "gS": leaves[0].grad, "gZ": leaves[1].grad, "g_h1": leaves[2].grad, "g_h2": leaves[3].grad}


def _against_restatement(h1, h2, init, beta, n, tag, views=None):
    """Clusterator + discriminator forward and backward, the Clusterator's backward from given gradients and the
    discriminator alone, against the restatement's autograd in fp64, bounded by the restatement in fp32.  h1, h2, init:
    fp32 CPU tensors; views: optional function turning the device copies into the layout under test (views.layout
    asserts it on every tensor that reaches s3grl_amd.gic, upstream gradients included)."""
    gic = _gic()
    gen = torch.Generator().manual_seed(11)
    N, d, K = h1.shape[0], h1.shape[1], init.shape[0]
    w = torch.randn(2 * N, generator=gen)
    S0 = torch.softmax(torch.randn((N, K), generator=gen), 1)
    Z0 = torch.randn((K, d), generator=gen)
    gZ0 = torch.randn((K, d), generator=gen)
    gS0 = torch.randn((N, K), generator=gen)
    cpu = (h1, h2, init, w, S0, Z0, gZ0, gS0)
    dev = [t.to(DEV) for t in cpu]
    layout = None
    if views is not None:
        dev, layout = views(dev), views.layout
    d_h1, d_h2, d_init, d_w, d_S0, d_Z0, d_gZ0, d_gS0 = dev
    got = _kernel_pass(gic.clusterator, gic.cluster_discriminator, d_h1, d_h2, d_init, beta, d_w, layout)
    got_c = _cluster_pass(gic.clusterator, d_h1, d_init, beta, d_gZ0, d_gS0, layout)
    got_d = _disc_pass(gic.cluster_discriminator, d_S0, d_Z0, d_h1, d_h2, d_w, layout)
    want, want_c, want_d = [], [], []
    for dt in (torch.float64, torch.float32):
        a = [t.to(dt) for t in cpu]
        want.append(_kernel_pass(R.clusterator, R.cluster_discriminator, a[0], a[1], a[2], beta, a[3]))
        want_c.append(_cluster_pass(R.clusterator, a[0], a[2], beta, a[6], a[7]))
        want_d.append(_disc_pass(R.cluster_discriminator, a[4], a[5], a[0], a[1], a[3]))
    for k in got:
        _hold(f"{tag} {k}", got[k], want[0][k], want[1][k], n)
    for k in got_c:
        _hold(f"{tag} cluster {k}", got_c[k], want_c[0][k], want_c[1][k], n)
    for k in got_d:
        _hold(f"{tag} disc {k}", got_d[k], want_d[0][k], want_d[1][k], n)


@pytest.mark.parametrize("case", R.CASES)
def test_cluster_backward_and_discriminator(case):
    g, o64, _ = _case(case)
    _against_restatement(o64["h1"].float(), o64["h2"].float(), torch.as_tensor(g["p_init"]).float(), float(g["beta"]),
                         _size(g), case)


@pytest.mark.parametrize("case", R.CASES)
def test_teacher_forced_step(case):
    from s3grl_amd.propagate import GicGraph

    gic = _gic()
    g, o64, o32 = _case(case)
    n_nodes, d, K = int(g["num_nodes"]), int(g["dim"]), int(g["K"])
    n = _size(g)
    x = None if int(g["x_is_eye"]) else torch.as_tensor(g["x"]).float().to(DEV)
    net = gic.GICTwin(n_nodes, n_nodes if x is None else x.shape[1], d, K, float(g["beta"]))
    net.load_state_dict(R.golden_state(g, torch.float32))
    net = net.to(DEV).train()
    graph = GicGraph(g["arcs"].T, n_nodes, DEV)
    logits, logits2 = net(x, torch.as_tensor(g["perm"]).to(DEV), graph)
    assert logits.shape == logits2.shape == (1, 2 * n_nodes)
    loss = gic.gic_loss(logits, logits2, float(g["alpha"]))
    loss.backward()
    got = {"logits": logits, "logits2": logits2, "loss": loss}
    got.update({"g_" + k: p.grad for k, p in net.named_parameters()})
    assert set(got) >= {"g_" + k for k in R.PARAMS}
    for k, v in got.items():
        _hold_golden(g, k, v, n)
        _hold(k + " (whole)", v, o64[k], o32[k], n)
    net.eval()
    h1, H, c, Z = net.embed(x, graph)
    for k, v in (("h1", h1), ("embed_H", H), ("embed_c", c), ("Z", Z)):
        _hold_golden(g, k, v, n)


# ---- layout sweep --------------------------------------------------------------------------------------------------
# (N, K, d): every d of {1, 3, 4, 32, 33, 100, 256}, every K of {1, 2, 10, 32, 128} and 64 / 65 on both sides of the
# K tile, every N of {1, 63, 64, 65} and 129 (three 64-node chunks: the multi-chunk reduction), and the declared limits
# K = 256 (four K tiles, the two backward kernels' 145 KiB of dynamic LDS) and d = 4096
SWEEP = [(1, 1, 1), (63, 2, 3), (64, 10, 4), (65, 32, 32), (129, 64, 33), (65, 65, 100), (64, 128, 256), (129, 10, 256),
         (1, 10, 32), (63, 128, 33), (129, 1, 100), (65, 2, 4), (129, 65, 3), (65, 256, 512), (3, 2, 4096)]


def _paths(N, K, d):
    from s3grl_amd.gic import CHUNK, TILE

    return {("chunks", min(-(-N // CHUNK), 2)), ("k_tiles", min(-(-K // TILE), 2)), ("d_tiles", min(-(-d // TILE), 2)),
            ("dot_tiles", min(-(-d // 32), 2))}


def test_sweep_reaches_every_path():
    """The kernels are not templated: one instance each.  Their paths are the loop trip counts: one or several node
    chunks (the partial reduction), K tiles, d tiles of the products, reduction tiles of dot_rows."""
    seen = set().union(*(_paths(*s) for s in SWEEP))
    from s3grl_amd import _native

    assert seen == {(p, c) for p in ("chunks", "k_tiles", "d_tiles", "dot_tiles") for c in (1, 2)}
    assert max(s[1] for s in SWEEP) == _native.GIC_MAX_CLUSTERS and max(s[2] for s in SWEEP) == _native.GIC_MAX_DIM
    assert {s[2] for s in SWEEP} >= {1, 3, 4, 32, 33, 100, 256}
    assert {s[1] for s in SWEEP} >= {1, 2, 10, 32, 64, 65, 128}
    assert {s[0] for s in SWEEP} >= {1, 63, 64, 65, 129}


def _sweep_inputs(N, K, d):
    gen = torch.Generator().manual_seed(1000 * N + 10 * K + d)
    return (torch.randn((N, d), generator=gen), torch.randn((N, d), generator=gen), torch.rand((K, d), generator=gen))


@pytest.mark.parametrize("N,K,d", SWEEP)
def test_layout_sweep(N, K, d):
    h1, h2, init = _sweep_inputs(N, K, d)
    _against_restatement(h1, h2, init, 10.0, N + K + d, f"N{N} K{K} d{d}")


def _strided_copy(t):
    """A copy of t that is not contiguous: column-major for a matrix, every second element of a buffer for a vector."""
    if t.dim() == 2:
        return t.t().contiguous().t()
    v = torch.empty(2 * t.numel(), dtype=t.dtype, device=t.device)[::2]
    v.copy_(t)
    return v


def _column_slices(dev):
    """h1 and h2 as the column halves of one [N, 2d] tensor (the twin's layout), everything else a strided copy."""
    h1, h2 = dev[0], dev[1]
    hh = torch.cat([h1, h2], 1)
    d = h1.shape[1]
    return [hh[:, :d], hh[:, d:]] + [_strided_copy(t) for t in dev[2:]]


def _is_strided(name, t):
    assert not t.is_contiguous(), name


def _misaligned(dev):
    """Every tensor contiguous and starting 4 bytes past a 16-byte boundary."""
    out = []
    for t in dev:
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        out.append(v)
    return out


def _is_misaligned(name, t):
    assert t.is_contiguous() and t.data_ptr() % 16 == 4, (name, t.data_ptr() % 16)


_column_slices.layout = _is_strided
_misaligned.layout = _is_misaligned


@pytest.mark.parametrize("views", [_column_slices, _misaligned])
@pytest.mark.parametrize("N,K,d", [(65, 10, 33), (129, 65, 100)])
def test_non_contiguous_and_misaligned_inputs(N, K, d, views):
    h1, h2, init = _sweep_inputs(N, K, d)
    _against_restatement(h1, h2, init, 10.0, N + K + d, views.__name__, views)


def test_shape_limits_raise_on_the_device():
    from s3grl_amd import _native

    gic = _gic()
    with pytest.raises(ValueError, match=str(_native.GIC_MAX_CLUSTERS)):
        gic.clusterator(torch.zeros((4, 8), device=DEV), torch.ones((_native.GIC_MAX_CLUSTERS + 1, 8), device=DEV), 10)
    with pytest.raises(ValueError):
        gic.clusterator(torch.zeros((4, 8), device=DEV), torch.ones((3, 7), device=DEV), 10)
    with pytest.raises(ValueError):
        gic.clusterator(torch.zeros((4, 8), device=DEV, dtype=torch.float64), torch.ones((3, 8), device=DEV), 10)


# ---- determinism and the loop --------------------------------------------------------------------------------------
def test_forward_backward_bit_identical():
    gic = _gic()
    h1, h2, init = (t.to(DEV) for t in _sweep_inputs(129, 65, 100))
    w = torch.randn(2 * 129, generator=torch.Generator().manual_seed(3)).to(DEV)
    a = _kernel_pass(gic.clusterator, gic.cluster_discriminator, h1, h2, init, 100.0, w)
    b = _kernel_pass(gic.clusterator, gic.cluster_discriminator, h1, h2, init, 100.0, w)
    assert all(torch.equal(a[k], b[k]) for k in a)


def _usair():
    from s3grl_amd import workloads

    n, e = workloads.load_topology("usair")
    return workloads.edge_split(n, e, seed=1)


def _lists(split):
    return [split.links["test"][0], split.links["test"][1], split.links["valid"][0], split.links["valid"][1]]


def test_calgic_is_deterministic():
    gic = _gic()
    split = _usair()
    args = gic.reference_args("usair", epochs=8, seed=3)
    runs = [gic.CalGIC(split.edge_index(), None, "usair", _lists(split), args, num_nodes=split.num_nodes)
            for _ in range(2)]
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])
    assert runs[0][1].shape == (split.num_nodes, 32) and runs[0][1].dtype == torch.float32 and not runs[0][1].is_cuda


def test_calgic_takes_its_hyper_parameters_from_args_data_name():
    gic = _gic()
    split = _usair()
    for data_name, want in (("pubmed", (10, 0.75, 32)), ("usair", (100, 0.5, 10))):
        trace = {}
        args = gic.reference_args(data_name, epochs=1, embedding_dim=8)
        gic.CalGIC(split.edge_index(), None, "cora", _lists(split), args, num_nodes=split.num_nodes, trace=trace)
        assert trace["hyper_parameters"] == want


def test_loop_steps_only_when_the_loss_did_not_improve():
    gic = _gic()
    g = R.golden("rand300")
    n, epochs = int(g["num_nodes"]), 6
    x = torch.as_tensor(g["x"]).float()
    gen = torch.Generator().manual_seed(9)
    perms = torch.stack([torch.randperm(n, generator=gen) for _ in range(epochs)])
    pairs = torch.as_tensor(g["arcs"][:40].T)
    lists = [pairs, pairs.flip(0), pairs, pairs.flip(0)]
    sd = R.golden_state(g, torch.float32)
    kw = dict(epochs=epochs, lr=0.01, permutations=perms, state_dict=sd)
    for every in (False, True):
        _, _, want = R.train_loop(g["arcs"].T, x, n, lists, "usair", dim=32, step_every_epoch=every, **kw)
        _, _, ref32 = R.train_loop(g["arcs"].T, x, n, lists, "usair", dim=32, step_every_epoch=every,
                                   dtype=torch.float32, **kw)
        trace = {}
        gic.train(g["arcs"].T, x, "usair", lists, embedding_dim=32, step_every_epoch=every, trace=trace, **kw)
        print("stepped", trace["stepped"], "restatement", want["stepped"])
        assert trace["stepped"] == want["stepped"]
        assert (trace["stepped"] == list(range(epochs))) if every else (0 not in trace["stepped"])
        _hold("losses", torch.tensor(trace["loss"]), torch.tensor(want["loss"]), torch.tensor(ref32["loss"]),
              n + 32 + 10)


def test_usair_row_end_to_end():
    gic = _gic()
    split = _usair()
    got = gic.run_gic(split, "usair")
    ref = []
    for seed in range(3):
        results, _, _ = R.train_loop(split.edge_index(), None, split.num_nodes, _lists(split), "usair", epochs=50,
                                     lr=0.01, dim=32, seed=seed, dtype=torch.float32)
        ref.append(R.best_at_first_max(results["AUC"])[1])
    margin = max(max(ref) - min(ref), 0.01)
    print(f"engine test AUC {got['AUC'][1]:.4f} (seed 1)  restatement {ref}  margin {margin:.4f}")
    assert got["AUC"][1] >= ref[1] - margin
    assert 0.0 <= got["AP"][1] <= 1.0


def test_init_gic_features():
    from s3grl_amd import workloads

    split = _usair()
    a = workloads.init_gic_features(split, None, 16, 5, "usair", seed=2)
    b = workloads.init_gic_features(split, None, 16, 5, "usair", seed=2)
    assert a.shape == (split.num_nodes, 16) and a.dtype == np.float32 and np.isfinite(a).all()
    assert a.min() == 0 and (a.sum(1) <= 1 + 1e-5).all()           # NormalizeFeatures: global min 0, row sums <= 1
    assert np.array_equal(a, b)
