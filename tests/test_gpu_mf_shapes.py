"""MF step kernels at every lane layout (csrc/s3grl_mf.hip): three teacher-forced steps against the fp64 restatement
(tests/mf_reference.py) on the table, every layer and both moment sets of each, and the loss, inside the bounds that
tests/mf_checks.py derives from Σ|terms|.  70 nodes; node 0 is in three pairs of four, on both sides; one self-pair,
one pair listed twice, one node in no pair.  tests/test_mf_host.py asserts that the shape list reaches every layout and
that every plausible kernel fault lands far outside these bounds."""
import numpy as np
import pytest

import mf_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: "H%d-L%d-B%s" % (s[0], s[1], "tile+1" if s[2] < 0 else s[2]))
def test_three_teacher_forced_steps_match_fp64(shape):
    from s3grl_amd import mf as M

    H, L, B = K.resolve(shape, M.layout)
    p = 0.5
    rng = np.random.default_rng(1000 * H + 10 * L + B)
    x0, layers0 = K.init_params(K.HUB_N, H, L, seed=H + L)
    mf = M.MFTrainer(K.HUB_N, H, L, p, 0.01, seed=0, init=(x0, layers0))
    st = mf.state()
    assert np.array_equal(st["weight"].cpu().numpy(), x0)                       # init= is read back bit for bit
    for (W, b), (W0, b0) in zip(st["layers"], layers0):
        assert np.array_equal(W.cpu().numpy(), W0) and np.array_equal(b.cpu().numpy(), b0)
    worst = {}
    for step in range(3):
        pos, neg = K.hub_pairs(B, rng)
        K.step_check(mf, pos, neg, K.random_masks(B, L, H, p, rng), p, worst, f"{shape} step {step}")
    print(shape, {k: f"{v:.2g}" for k, v in worst.items()})
    got = K.state_of(mf)
    assert not got["xm"][K.HUB_N - 1].any() and np.array_equal(got["x"][K.HUB_N - 1], x0[K.HUB_N - 1])
    mf.close()
