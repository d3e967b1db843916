#!/usr/bin/env python3
"""Generate tests/golden/linkclf_*.npz — sklearn-pinned fits of the link classifier.  Run on the CPU where sklearn is
installed (`python tests/golden/make_linkclf_golden.py`); the tests that read the files need neither sklearn nor a GPU.

Per case an fp32 table, a pair list and labels (tests/linkclf_checks.make_input), and what
`sklearn.linear_model.LogisticRegression` makes of the Hadamard features emb[src] * emb[dst]:
    emb [70, D] fp32, pairs [M, 2] int64, labels [M] uint8
    default_coef [D], default_intercept, default_predict [M]   LogisticRegression() on the fp32 features, as the
                                                                reference baselines/n2v.py fits it
    tight_coef [D], tight_intercept, tight_predict [M]         LogisticRegression(tol=1e-12, max_iter=100000) on the
                                                                same products in fp64 (they are exact there)
    sklearn_version
The GPU test compares hard predictions with default_predict and leaves out only the rows where default_predict and
tight_predict differ in the file itself; at most 1 % of a case's rows may differ, or this script fails."""
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import linkclf_checks as K  # noqa: E402

CASES = {"d8": dict(D=8, M=40, seed=11), "d32": dict(D=32, M=600, seed=12), "d33": dict(D=33, M=257, seed=13)}


def main():
    import sklearn
    from sklearn.linear_model import LogisticRegression

    for name, kw in CASES.items():
        emb, pairs, y = K.make_input(**kw)
        x32 = emb[pairs[:, 0]] * emb[pairs[:, 1]]
        x64 = emb[pairs[:, 0]].astype(np.float64) * emb[pairs[:, 1]].astype(np.float64)
        default = LogisticRegression().fit(x32, y)
        tight = LogisticRegression(tol=1e-12, max_iter=100000).fit(x64, y)
        dp, tp = default.predict(x32).astype(np.uint8), tight.predict(x64).astype(np.uint8)
        differ = int((dp != tp).sum())
        assert differ <= 0.01 * len(y), f"{name}: {differ} of {len(y)} rows differ between default and tight sklearn"
        np.savez_compressed(HERE / f"linkclf_{name}.npz", emb=emb, pairs=pairs, labels=y,
                            default_coef=default.coef_[0].astype(np.float64),
                            default_intercept=np.float64(default.intercept_[0]), default_predict=dp,
                            tight_coef=tight.coef_[0].astype(np.float64),
                            tight_intercept=np.float64(tight.intercept_[0]), tight_predict=tp,
                            sklearn_version=np.array(sklearn.__version__))
        print(f"linkclf_{name}.npz: D {kw['D']}, M {kw['M']}, {differ} rows differ, "
              f"max|default - tight| {np.max(np.abs(default.coef_ - tight.coef_)):.1e}")


if __name__ == "__main__":
    main()
