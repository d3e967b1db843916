"""The link-classifier kernels at every lane layout and tile edge (csrc/s3grl_linkclf.hip): per shape three
teacher-forced Newton steps against the float64 restatement (tests/linkclf_reference.py) on the gradient, the loss, the
rung, the direction and the new θ, then a full fit against θ* and the restatement's n_iter, and predict /
decision_function / confusion on the fitted rows, all inside the bounds that tests/linkclf_checks.py derives from
Σ|terms|.  70 nodes; node 0 is in three pairs of four, on both sides; one self-pair, one pair listed twice with both
labels, one node in no pair.  tests/test_linkclf_host.py asserts that the shape list reaches every layout and tile edge,
that the restatement's own decisions on it are clear of rounding, and that every plausible kernel fault lands far outside
these bounds."""
import numpy as np
import pytest

import linkclf_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", K.DIMS)
def test_steps_fit_and_predictions_match_fp64(D):
    from s3grl_amd import linkclf as L

    worst = {}
    for M in K.row_counts(L.layout(D)["rows_per_block"]):
        emb, pairs, y = K.make_input(D, M, seed=1)
        tag = f"D {D} M {M}"
        clf = L.LinkClassifier(D)
        assert not clf.state()["theta"].any()                         # a fresh classifier stands at θ = 0
        for step in range(3):
            K.step_check(clf, emb, pairs, y, worst, f"{tag} step {step}")
        theta, ref = K.fit_check(clf, emb, pairs, y, worst, tag)      # fit starts again from 0
        again = L.LinkClassifier(D)
        again.fit(emb, pairs, y)
        assert np.array_equal(np.r_[again.coef_[0], again.intercept_], theta), f"{tag}: two fits differ"
        # the launches after `done` change nothing: a fit with exactly the iterations needed is bit-identical
        short = L.LinkClassifier(D, max_iter=ref["n_iter"] + 1)
        short.fit(emb, pairs, y)
        assert short.converged_ and np.array_equal(np.r_[short.coef_[0], short.intercept_], theta), tag
        for c in (clf, again, short):
            c.close()
    print(D, {k: f"{v:.2g}" for k, v in worst.items()})
