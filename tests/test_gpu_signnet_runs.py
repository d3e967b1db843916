"""The runs of a config trained side by side on the MI355X (s3grl_amd.signnet.SIGNNetRuns, the signnet_*_runs_kernel
group kernels of csrc/s3grl_signnet.hip): every member of a group is bit-identical to the lone `SIGNNetTrainer` of its
seed, dropout and lr (parameters, Adam's moments and count, running statistics, losses and scores), at every
instantiation of the step kernels and at the size edges, and stays an ordinary trainer before and after a group epoch.
No tolerance anywhere: `_same` is torch.equal on `state_dict(optimizer=True)`."""
import ctypes as C

import pytest
import torch

import signnet_checks as K

pytestmark = pytest.mark.gpu


def _same(a, b):
    sa, sb = a.state_dict(optimizer=True), b.state_dict(optimizer=True)
    return sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) if isinstance(sa[k], torch.Tensor) else sa[k] == sb[k]
                                          for k in sa)


def _store(kind, in_width, seed):
    return tuple(torch.as_tensor(t).cuda() for t in K.make_store(kind, in_width, seed))


def _close(*things):
    for t in things:
        t.close()


def test_every_member_is_the_lone_trainer_of_its_seed():
    from s3grl_amd.signnet import SIGNNetRuns, SIGNNetTrainer

    H, IW, B = 32, 64, 32
    x, row_ptr, y = _store("mixed", IW, 5)                  # 70 links: steps of 32, 32 and 6; link 37 has 72 rows
    seeds, drop, lr = (21, 22, 23), (0.5, 0.5, 0.0), (1e-3, 1e-3, 2e-3)
    group = SIGNNetRuns(IW, H, 1, "mean", drop, lr, seeds=seeds)
    assert [m.seed for m in group.members] == list(seeds) and all(isinstance(m, SIGNNetTrainer) for m in group.members)
    losses = [group.fit_epoch(x, row_ptr, y, B) for _ in range(2)]
    assert losses[0].shape == (3, 3) and losses[0].dtype == torch.float32 and not losses[0].is_cuda
    assert bool(torch.isfinite(torch.stack(losses)).all())
    scores = group.score(x, row_ptr)
    assert scores.shape == (3, 70) and scores.is_cuda
    for r, (seed, p, rate) in enumerate(zip(seeds, drop, lr)):
        lone = SIGNNetTrainer(IW, H, 1, "mean", p, rate, seed=seed)
        for e in range(2):
            assert torch.equal(lone.fit_epoch(x, row_ptr, y, B), losses[e][r]), (r, e)
        assert _same(group.members[r], lone), r
        assert torch.equal(lone.score(x, row_ptr), scores[r]), r
        lone.close()
    sd = group.state_dict(optimizer=True)
    assert sd[0]["step"] == 6 and int(sd[2]["link_pred_mlp.2.num_batches_tracked"]) == 6
    assert group.epochs_done == 2 and all(m.epochs_done == 2 for m in group.members)
    assert not torch.equal(sd[0]["operator_diff.0.weight"], sd[1]["operator_diff.0.weight"])
    assert not torch.equal(losses[0][0], losses[0][1]) and not torch.equal(scores[0], scores[1])
    group.close()


# (the SHAPES row, the runs of the group): H = 1 with steps of two links, the largest group, a pooled head that is not a
# multiple of 4 wide, H one below the limit with a step of 4 links left over, and H = 256 with five runs (320
# workgroups per launch, more than the chip has CUs).  Those five reach the layouts (1, 1), (4, 1) and (4, 4); the sixth
# row is there for (1, 4): scalar loads along in_width = 65, float4 loads along the head's 32 inputs.
GROUP_SHAPES = [((1, 1, 2, 0.0, "", "two"), 2), ((7, 65, 33, 0.5, "sum", "mixed"), 16),
                ((33, 64, 64, 0.0, "mean", "mixed"), 3), ((255, 3, 33, 0.5, "", "two"), 2),
                ((256, 2004, 32, 0.5, "mean", "mixed"), 5), ((32, 65, 64, 0.5, "", "mixed"), 2)]


def test_the_group_shapes_reach_every_layout():
    from s3grl_amd import signnet

    assert all(shape in K.SHAPES for shape, _ in GROUP_SHAPES)
    seen = set()
    for (H, IW, B, _, mode, _), _ in GROUP_SHAPES:
        lay = signnet.layout(H, IW, B, bool(mode))
        seen.add((lay["k_vector"], lay["head_k_vector"]))
    assert seen == K.LAYOUTS
    assert max(R for _, R in GROUP_SHAPES) == 16
    assert any(R * signnet.layout(s[0], s[1], s[2], bool(s[4]))["workgroups"] > 256 for s, R in GROUP_SHAPES)


@pytest.mark.parametrize("shape,R", GROUP_SHAPES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_one_group_epoch_at_every_instantiation_and_size_edge(shape, R):
    from s3grl_amd.signnet import SIGNNetRuns, SIGNNetTrainer

    H, IW, B, p, mode, kind = shape
    x, row_ptr, y = _store(kind, IW, K.SEEDS[shape])
    kh = 1 if mode else 0
    seeds = [100 + 7 * r for r in range(R)]
    group = SIGNNetRuns(IW, H, kh, mode, p, 1e-3, seeds=seeds)
    losses = group.fit_epoch(x, row_ptr, y, B)
    steps = -(-(K.NUM_LINKS - 1) // B)
    assert losses.shape == (R, steps)
    scores = group.score(x, row_ptr)
    for r, seed in enumerate(seeds):
        lone = SIGNNetTrainer(IW, H, kh, mode, p, 1e-3, seed=seed)
        assert torch.equal(lone.fit_epoch(x, row_ptr, y, B), losses[r]), (shape, r)
        assert _same(group.members[r], lone), (shape, r)
        assert torch.equal(lone.score(x, row_ptr), scores[r]), (shape, r)
        lone.close()
    group.close()


def test_a_group_of_one_is_the_lone_trainer():
    from s3grl_amd.signnet import SIGNNetRuns, SIGNNetTrainer

    H, IW, B = 32, 64, 32
    x, row_ptr, y = _store("mixed", IW, 5)
    group, lone = SIGNNetRuns(IW, H, 1, "sum", 0.5, 1e-3, seeds=(9,)), SIGNNetTrainer(IW, H, 1, "sum", 0.5, 1e-3, seed=9)
    for _ in range(2):
        got = group.fit_epoch(x, row_ptr, y, B)
        assert got.shape == (1, 3) and torch.equal(got[0], lone.fit_epoch(x, row_ptr, y, B))
    assert _same(group.members[0], lone)
    _close(group, lone)


def test_adams_count_is_each_members_own():
    from s3grl_amd.signnet import SIGNNetRuns, SIGNNetTrainer

    H, IW, B = 32, 64, 32
    x, row_ptr, y = _store("mixed", IW, 5)
    donor = SIGNNetTrainer(IW, H, 1, "mean", 0.5, 1e-3, seed=3)
    donor.fit_epoch(x, row_ptr, y, B)
    sd = donor.state_dict(optimizer=True)                    # non-zero moments, running statistics of three steps
    assert float(sd["exp_avg.operator_diff.0.weight"].abs().max()) > 0 and sd["step"] == 3
    sd["step"] = 5
    group = SIGNNetRuns(IW, H, 1, "mean", 0.5, 1e-3, seeds=(31, 32, 33))
    group.members[1].load_state_dict(sd)
    lones = [SIGNNetTrainer(IW, H, 1, "mean", 0.5, 1e-3, seed=s, init=sd if s == 32 else None) for s in (31, 32, 33)]
    assert _same(group.members[1], lones[1]) and group.members[1].state_dict(optimizer=True)["step"] == 5
    losses = group.fit_epoch(x, row_ptr, y, B)
    for r, lone in enumerate(lones):
        assert torch.equal(lone.fit_epoch(x, row_ptr, y, B), losses[r]), r
        assert _same(group.members[r], lone), r
    counts = [m.state_dict(optimizer=True)["step"] for m in group.members]
    assert counts == [3, 8, 3]
    _close(group, donor, *lones)


def test_members_and_lone_trainers_are_interchangeable():
    from s3grl_amd.signnet import SIGNNetRuns, SIGNNetTrainer

    H, IW, B = 32, 64, 32
    x, row_ptr, y = _store("mixed", IW, 5)
    group = SIGNNetRuns(IW, H, 1, "mean", 0.5, 1e-3, seeds=(41, 42, 43))
    losses = group.fit_epoch(x, row_ptr, y, B)
    # a member goes on alone where a lone trainer would
    lone = SIGNNetTrainer(IW, H, 1, "mean", 0.5, 1e-3, seed=41)
    lone.fit_epoch(x, row_ptr, y, B)
    assert torch.equal(group.members[0].fit_epoch(x, row_ptr, y, B), lone.fit_epoch(x, row_ptr, y, B))
    assert _same(group.members[0], lone)
    # a lone twin replays group epoch 0 of member 2 through the teacher-forcing hook
    twin = SIGNNetTrainer(IW, H, 1, "mean", 0.5, 1e-3, seed=43)
    for step in range(3):
        ids, m1, m2 = twin.draws(0, step, 70, B, row_ptr)
        loss = twin.step(x, row_ptr, y, ids, m1, m2)
        assert torch.tensor(loss, dtype=torch.float32) == losses[2][step], step
    assert _same(group.members[2], twin)
    # and the member's own draws are those of its seed
    for a, b in zip(group.members[2].draws(1, 2, 70, B, row_ptr), twin.draws(1, 2, 70, B, row_ptr)):
        assert torch.equal(a, b)
    _close(group, lone, twin)


def test_errors():
    from s3grl_amd import _native as N
    from s3grl_amd.signnet import SIGNNetRuns, SIGNNetTrainer

    H, IW, B = 8, 12, 32
    x, row_ptr, y = _store("two", IW, 1)
    with pytest.raises(NotImplementedError, match="16"):
        SIGNNetRuns(IW, H, seeds=range(17))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SIGNNetRuns(IW, H, seeds=(1, 2), device="cpu")
    group = SIGNNetRuns(IW, H, seeds=(1, 2, 3))
    group.fit_epoch(x, row_ptr, y, B)
    group.members[1].fit_epoch(x, row_ptr, y, B)            # advanced alone: the counters disagree
    before = group.state_dict(optimizer=True)
    with pytest.raises(ValueError, match="epoch"):
        group.fit_epoch(x, row_ptr, y, B)
    after = group.state_dict(optimizer=True)                # nothing was trained by the refused call
    assert all(torch.equal(a[k], b[k]) for a, b in zip(before, after) for k in a if isinstance(a[k], torch.Tensor))
    group.close()
    group = SIGNNetRuns(IW, H, seeds=(1, 2, 3))
    group.members[2].close()
    with pytest.raises((ValueError, RuntimeError), match="closed"):
        group.fit_epoch(x, row_ptr, y, B)
    with pytest.raises((ValueError, RuntimeError), match="closed"):
        group.score(x, row_ptr)
    with pytest.raises(ValueError, match="one state dict per member"):
        group.load_state_dict([])
    group.close()

    # the C call: members of one shape and context, every handle once
    a, b, wide, deep, pooled = (SIGNNetTrainer(IW, H, seed=1), SIGNNetTrainer(IW, H, seed=2),
                                SIGNNetTrainer(IW, H + 1, seed=3), SIGNNetTrainer(IW + 1, H, seed=4),
                                SIGNNetTrainer(IW, H, 1, "mean", seed=5))

    def call(*members):
        R = len(members)
        handles, lr = (C.c_void_p * R)(*[m._h.value for m in members]), (C.c_double * R)(*([1e-3] * R))
        return N.lib().s3grl_signnetruns_fit_epoch(handles, R, 0, N.ptr(x), x.shape[0], N.ptr(row_ptr), N.ptr(y),
                                                     y.numel(), B, lr, None)

    for bad in ((a, wide), (a, deep), (a, pooled), (a, b, a)):
        assert call(*bad) == N.ERR_INVALID_ARGUMENT
        assert "signnet group" in N.lib().s3grl_last_error().decode()
    assert a.state_dict(optimizer=True)["step"] == 0
    assert call(a, b) == N.OK                               # (and a null step_loss is allowed)
    assert a.state_dict(optimizer=True)["step"] == 3 == b.state_dict(optimizer=True)["step"]
    _close(a, b, wide, deep, pooled)


@pytest.mark.parametrize("eval_metric", ["auc", "hits"])
def test_fit_and_select_runs_is_fit_and_select_per_seed(eval_metric):
    from s3grl_amd.harness import fit_and_select, fit_and_select_runs, run_statistics

    H, IW = 32, 64
    train, valid, test = ((x.view(x.shape[0], 2, IW // 2), ptr, y) for x, ptr, y in
                          (_store("mixed", IW, s) for s in (5, 6, 7)))
    kw = dict(eval_metric=eval_metric, k_heuristic=1, k_pool_strategy="mean", hidden=H, epochs=2, lr=1e-3)
    out = fit_and_select_runs(train, valid, test, runs=3, seed=4, **kw)
    assert set(out) == {"runs", "statistics", "trainer"} and len(out["runs"]) == 3
    assert out["trainer"].seeds == (4, 5, 6) and out["trainer"].epochs_done == 2
    for r, got in enumerate(out["runs"]):
        want = fit_and_select(train, valid, test, seed=4 + r, **kw)
        want.pop("trainer").close()
        assert set(got) == {"history", "best_epoch", "selected"}
        assert got == want, r
        assert all(len(h) == 2 for h in got["history"].values())
    assert out["statistics"] == run_statistics([run["history"] for run in out["runs"]])      # (three runs: no NaN)
    keys = {"auc": {"AUC", "AP"}, "hits": {"Hits@20", "Hits@50", "Hits@100"}}[eval_metric]
    assert set(out["statistics"]) == keys
    for s in out["statistics"].values():
        assert len(s["per_run"]) == 3 and s["highest_test"]["std"] == s["highest_test"]["std"]      # three runs: no NaN
    out["trainer"].close()
