"""The fused SIGNNet step on the MI355X (s3grl_amd.signnet, csrc/s3grl_signnet.hip) against the fp64 restatement
(tests/signnet_reference.py) at every layout and edge: three teacher-forced steps per shape on every parameter,
exp_avg, exp_avg_sq, both BatchNorms' running statistics and the loss, then `score` on the whole store (70 links: one
more than a score tile) and on a store of one link.  The bounds are measured from the restatement itself
(tests/signnet_checks.py)."""
import numpy as np
import pytest
import torch

import signnet_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_three_teacher_forced_steps_and_score(shape):
    from s3grl_amd.signnet import SIGNNetTrainer

    H, IW, B, p, mode, kind = shape
    case = K.Case(H, IW, B, p, mode, kind, K.SEEDS[shape])
    net = SIGNNetTrainer(IW, H, k_heuristic=1 if mode else 0, k_pool_strategy=mode, dropout=p, lr=case.lr, seed=0,
                         init=K.twin_state_dict(case.params))
    worst = {}
    for i, (ids, m1, m2) in enumerate(case.batches(3)):
        K.step_check(net, case.store, ids, m1, m2, p, mode, worst, f"{shape} step {i}")
    x, row_ptr, _ = case.store
    st = K.state_of(net)
    for name, (xs, ptr) in (("store", (x, row_ptr)), ("one link", (x[:row_ptr[1]], row_ptr[:2]))):
        ref, bound = K.score_bounds(st, xs, ptr, mode)
        got = net.score(torch.as_tensor(xs), torch.as_tensor(ptr)).cpu().double().numpy()
        assert got.shape == ref.shape
        ratio = float(np.max(np.abs(got - ref) / bound))
        worst["score"] = max(worst.get("score", 0.0), ratio)
        assert ratio <= 1.0, f"{shape} score of the {name}: |engine - restatement| / bound = {ratio}"
    print("signnet worst ratio", shape, {k: round(v, 3) for k, v in worst.items()})
    net.close()
