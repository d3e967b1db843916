"""What the link-classifier tests share (tests/test_linkclf_host.py, tests/test_gpu_linkclf.py,
tests/test_gpu_linkclf_shapes.py, tests/test_gpu_n2v_row.py): the shape list, the input makers, the bounds of one
teacher-forced Newton step and of a fit against the float64 restatement (tests/linkclf_reference.py), the restatement
with one fault each, and the comparison the GPU tests run per shape.  Every bound is derived from Σ|terms| of a sum the
engine forms in fp64 (unit roundoff U = 2⁻⁵³; a sum of k terms in any order carries at most (k − 1) U Σ|terms|), pushed
through the first-order sensitivity of what is computed from it.  numpy only; nothing here needs a GPU until a classifier
object is passed in."""
from contextlib import contextmanager

import numpy as np

import linkclf_reference as R

U = 2.0 ** -53           # fp64 unit roundoff: the engine accumulates everything in fp64
U32 = 2.0 ** -24         # the decision values are handed out as fp32

# ---- shapes --------------------------------------------------------------------------------------------------------
# D covers every (channels per lane, lanes per row): 1, 2, 3 (4 lanes), 8, 16, 31 / 32 (32 lanes), 33 / 63 / 64 (64
# lanes, one channel each), 65 / 128 (two channels); D + 1 = 64, 65 and 129 straddle the wave and half the block.
DIMS = (1, 2, 3, 8, 16, 31, 32, 33, 63, 64, 65, 128)
LAYOUTS = {(1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (1, 32), (1, 64), (2, 64)}
HUB_N = 70


def row_counts(rows_per_block):
    """M of the shape list: 2, around a wave, around one tile, and four blocks with a one-row tail."""
    r = rows_per_block
    return sorted({2, 63, 64, 65, r - 1, r, r + 1, 3 * r + 1})


def many_tiles(lay):
    """The smallest M at which a block takes two tiles, plus a one-row tail."""
    return lay["max_blocks"] * lay["rows_per_block"] + lay["rows_per_block"] + 1


# ---- inputs --------------------------------------------------------------------------------------------------------
def hub_pairs(M, rng, n=HUB_N):
    """[M, 2] over n nodes: node 0 is an endpoint of three pairs in four, as src and as dst; from 4 pairs on row 3 is the
    self-pair (5, 5); from 8 on rows 6 and 7 are one pair (it gets both labels); node n - 1 is in no pair."""
    p = rng.integers(1, n - 1, size=(M, 2))
    i = np.arange(M)
    p[i % 4 == 0, 0] = 0
    p[i % 4 == 1, 1] = 0
    p[i % 4 == 2, 0] = 0
    if M >= 4:
        p[3] = (5, 5)
    if M >= 8:
        p[7] = p[6]
    return p


def make_input(D, M, seed, scale=1.0, separable=False, n=HUB_N):
    """(emb fp32 [n, D], pairs int64 [M, 2], labels uint8 [M]): an N(0, scale²) table, hub pairs, labels planted by a
    random direction plus noise (none when separable), about 60 % positives so that the intercept matters."""
    rng = np.random.default_rng([seed, D, M])
    emb = (rng.standard_normal((n, D)) * scale).astype(np.float32)
    pairs = hub_pairs(M, rng, n)
    x = R.features(emb, pairs)[:, :-1]
    s = x @ rng.standard_normal(D)
    if not separable:
        s = s + 0.7 * (np.std(s) + 1e-300) * rng.standard_normal(M)
    y = (s > np.quantile(s, 0.4)).astype(np.uint8)
    if M >= 8 and not separable:
        y[6], y[7] = 1, 0
    if y.min() == y.max():
        y[0], y[1] = 1, 0
    return emb, pairs, y


SEPARABLE = dict(D=8, M=65, seed=3, separable=True)      # only the ridge keeps θ finite
TINY_SCALE = dict(D=32, M=65, seed=4, scale=0.05)        # H is nearly the ridge alone
REJECTED = dict(D=32, M=193, seed=5)                     # from 20 θ* the full step is rejected


# ---- bounds --------------------------------------------------------------------------------------------------------
def row_bounds(Z, theta):
    """(z, w, dz, dr, dw): z, p(1 − p), and what an fp64 evaluation of z, of p − y and of p(1 − p) may differ by.  z is
    a sum of n products; p and p(1 − p) come from one exp, one division and products of values <= 1 (4 and 6
    roundoffs); their derivatives in z are p(1 − p) and p(1 − p)(1 − 2p)."""
    n = Z.shape[1]
    z, _, w, _ = R.row_terms(Z, np.zeros(len(Z)), theta)
    dz = (n + 1) * U * (np.abs(Z) @ np.abs(theta))
    return z, w, dz, w * dz + 4 * U, w * (dz + 6 * U)


def grad_bound(Z, y, theta, C):
    M = len(Z)
    z, r, w, l = R.row_terms(Z, y, theta)
    _, _, dz, dr, _ = row_bounds(Z, theta)
    g = C * (Z.T @ r) + R.ridge(len(theta)) * theta
    return C * ((M + 2) * U * (np.abs(Z).T @ np.abs(r)) + np.abs(Z).T @ dr) + 2 * U * np.abs(theta) + U * np.abs(g)


def loss_bound(Z, y, theta, C):
    M, n = Z.shape
    z, r, w, l = R.row_terms(Z, y, theta)
    _, _, dz, _, _ = row_bounds(Z, theta)
    dl = np.maximum(np.abs(r), 1.0) * dz + 4 * U * (np.abs(l) + np.abs(z))
    ww = 0.5 * float(np.sum(theta[:-1] ** 2))
    return C * ((M + 2) * U * float(np.sum(np.abs(l))) + float(np.sum(dl))) + (n + 2) * U * ww + \
        U * abs(ww + C * float(np.sum(l)))


def hess_bound(Z, y, theta, C, H):
    M = len(Z)
    _, w, _, _, dw = row_bounds(Z, theta)
    A = np.abs(Z)
    return C * ((M + 3) * U * ((A * w[:, None]).T @ A) + (A * dw[:, None]).T @ A) + U * np.abs(H)


def step_bounds(Z, y, ref, C):
    """Bounds of one iteration against `ref` = R.newton_step from the same θ: dict(g [n], f0, d [n], gtd, margins
    [RUNGS]).  d̂ solves (H + ΔH) d̂ = g + Δg with |ΔH| <= e_H + γ |Uᵀ||U|, γ = (3n + 1) U for a Cholesky solve
    (Higham, Accuracy and Stability, Thm 10.4), once for the engine and once for numpy's: |Δd| <= |H⁻¹| (e_g + (e_H + 2γ
    |Uᵀ||U|) |d|) to first order.  A ladder loss moves by its own rounding and by ∇f(θ − t d)·t Δd."""
    theta, n = ref["theta0"], Z.shape[1]
    b = {"g": grad_bound(Z, y, theta, C), "f0": loss_bound(Z, y, theta, C)}
    if "d" not in ref:
        return b
    d, Uf = ref["d"], np.abs(ref["U"])
    gamma = (3 * n + 1) * U
    Hinv = np.abs(np.linalg.inv(ref["H"]))
    b["d"] = Hinv @ (b["g"] + (hess_bound(Z, y, theta, C, ref["H"]) + 2 * gamma * (Uf.T @ Uf)) @ np.abs(d))
    b["gtd"] = float(b["g"] @ np.abs(d) + np.abs(ref["g"]) @ b["d"] + (n + 1) * U * (np.abs(ref["g"]) @ np.abs(d)))
    m = np.full(R.RUNGS, np.inf)            # past the first rung accepted for certain no rung is looked at
    for k, t in enumerate(R.LADDER):
        th = theta - t * d
        if not np.isfinite(ref["fk"][k]):
            continue
        gk = R.grad(Z, y, th, C)
        m[k] = loss_bound(Z, y, th, C) + t * float(np.abs(gk) @ b["d"]) + (1 + R.SLACK) * b["f0"] + R.C1 * t * b["gtd"]
        if ref["margins"][k] <= -m[k]:
            break
    b["margins"] = m
    return b


def allowed_rungs(margins, bound):
    """The rungs an evaluation within `bound` of `margins` may take: every k up to and including the first that is
    accepted for certain, that is not rejected for certain."""
    out = []
    for k in range(R.RUNGS):
        if margins[k] <= bound[k]:
            out.append(k)
        if margins[k] <= -bound[k]:
            return out
    return out + [R.RUNGS]


def fit_bound(Z, y, theta_star, gmax_star, C, tol):
    """max|θ̂ − θ*| of an iterate whose COMPUTED gradient is within tol: its true gradient is within tol + e_g, θ* has
    gmax_star left, and ∇f(θ̂) − ∇f(θ*) = H̄ (θ̂ − θ*) with H̄ the Hessian between them, which differs from H(θ*) by a
    relative O(|θ̂ − θ*|) (1e-6 covers it)."""
    H = R.grad_hess(Z, y, theta_star, C)[1]
    e_g = float(np.max(grad_bound(Z, y, theta_star, C)))
    return (1 + 1e-6) * float(np.linalg.norm(np.linalg.inv(H), np.inf)) * (tol + e_g + gmax_star)


def z_bound(Z, theta, theta_bound):
    """per row: what z may differ by when θ differs by theta_bound per element, plus the dot product's own rounding"""
    return np.abs(Z).sum(axis=1) * theta_bound + (Z.shape[1] + 1) * U * (np.abs(Z) @ np.abs(theta))


def unambiguous(Z, y, C, tol, init=None, max_iter=50):
    """The restatement's fit with every decision checked against its bound: (fit, True when no convergence test and no
    rung choice along the way could fall the other way within the engine's rounding).  The convergence test asks
    that max|∇f| differ from tol by more than one part in 1000: the iterates of two Newton runs agree to about 1e-12
    (step_bounds' d, and Newton's map contracts next to the optimum), nine orders below that."""
    r = R.fit(Z, y, C, tol, max_iter, init)
    clear = True
    for s in r["steps"]:
        if abs(s["gmax"] - tol) <= 1e-3 * tol:
            clear = False
        if "d" in s:
            b = step_bounds(Z, y, s, C)
            if len(allowed_rungs(s["margins"], b["margins"])) != 1:
                clear = False
    return r, clear


# ---- the comparison the GPU tests run ------------------------------------------------------------------------------
def _ratio(worst, name, value):
    worst[name] = max(worst.get(name, 0.0), float(value))
    return float(value)


def step_check(clf, emb, pairs, y, worst, tag):
    """One `clf.newton_step` against the restatement's step from the engine's own θ (teacher forcing): g, f, the rung,
    d (from the move) and the new θ inside step_bounds.  Updates worst {name: |engine − restatement| / bound}."""
    Z, yf = R.features(emb, pairs), np.asarray(y, dtype=np.float64)
    theta0 = clf.state()["theta"].copy()
    ref = R.newton_step(Z, yf, theta0, clf.C, clf.tol)
    b = step_bounds(Z, yf, ref, clf.C)
    s = clf.newton_step(emb, pairs, y)
    bad = {}
    r = {"g": np.max(np.abs(s["grad"] - ref["g"]) / b["g"]), "f": abs(s["loss"] - ref["f0"]) / b["f0"]}
    if "d" not in ref:                                   # converged (or a failed factorisation) in the restatement
        assert abs(ref["gmax"] - clf.tol) > np.max(b["g"]), f"{tag}: the convergence test is within rounding"
        assert s["done"] == ref["done"] and np.array_equal(s["theta"], theta0), f"{tag}: {s['done']} vs {ref['done']}"
    else:
        ok = allowed_rungs(ref["margins"], b["margins"])
        k = R.RUNGS if s["step_t"] == 0 else int(round(-np.log2(s["step_t"])))
        assert k in ok, f"{tag}: the engine took rung {k}, the restatement allows {ok}"
        assert k == ref["k"], f"{tag}: rung {k} vs {ref['k']} (both inside the bound: pick another seed)"
        if k < R.RUNGS:
            t = R.LADDER[k]
            r["d"] = np.max(np.abs((theta0 - s["theta"]) / t - ref["d"]) / (b["d"] + 2 * U * (np.abs(theta0) + np.abs(s["theta"])) / t))
            r["theta"] = np.max(np.abs(s["theta"] - ref["theta"]) / (t * b["d"] + 2 * U * np.abs(ref["theta"])))
    for name, v in r.items():
        if not _ratio(worst, name, v) <= 1.0:
            bad[name] = float(v)
    assert not bad, f"{tag}: |engine − restatement| / bound = {bad}"
    return s, ref


def fit_check(clf, emb, pairs, y, worst, tag, init=None):
    """A full `clf.fit` against θ* and the restatement's n_iter; then predict / decision_function / confusion on the
    same rows, exactly, but for rows whose |z| is inside the bound on z (there must be none)."""
    Z, yf = R.features(emb, pairs), np.asarray(y, dtype=np.float64)
    ref, clear = unambiguous(Z, yf, clf.C, clf.tol, init, clf.max_iter)
    assert clear and ref["done"] == R.CONVERGED, f"{tag}: the restatement's own decisions are within rounding"
    star, gstar = R.optimum(Z, yf, clf.C, init)
    tb = fit_bound(Z, yf, star, gstar, clf.C, clf.tol)
    clf.fit(emb, pairs, y, init=init)
    theta = np.r_[clf.coef_[0], clf.intercept_]
    assert clf.converged_ and clf.n_iter_ == ref["n_iter"], f"{tag}: n_iter {clf.n_iter_} vs {ref['n_iter']}"
    v = _ratio(worst, "fit_theta", np.max(np.abs(theta - star)) / tb)
    assert v <= 1.0, f"{tag}: |θ − θ*| / bound = {v}"
    zb = z_bound(Z, star, tb)
    zr = R.decision(Z, star)
    keep = np.abs(zr) > zb
    assert keep.all(), f"{tag}: {int((~keep).sum())} rows of the restatement lie inside the bound on z: another seed"
    pred = clf.predict(emb, pairs).cpu().numpy()
    assert pred.dtype == np.uint8 and np.array_equal(pred, R.predict(Z, star)), f"{tag}: predict"
    dec = clf.decision_function(emb, pairs).cpu().numpy().astype(np.float64)
    v = _ratio(worst, "decision", np.max(np.abs(dec - zr) / (zb + U32 * np.abs(zr))))
    assert v <= 1.0, f"{tag}: |decision − z| / bound = {v}"
    assert clf.confusion(emb, pairs, y) == R.confusion(R.predict(Z, star), y), f"{tag}: confusion"
    return theta, ref


# ---- the restatement with one fault --------------------------------------------------------------------------------
FAULTS = ("last_block_partial_dropped", "tail_rows_dropped", "intercept_penalised", "label_flipped",
          "last_column_dropped", "rung_off_by_one", "self_pair_as_zero")


@contextmanager
def _ridge_everywhere():
    keep = R.ridge
    R.ridge = lambda n: np.ones(n)
    try:
        yield
    finally:
        R.ridge = keep


def faulty_step(emb, pairs, y, theta, fault, rows_per_block, C=1.0, tol=1e-8):
    """R.newton_step from theta with one fault a kernel could have: dict(g, f0, theta).  None when the input cannot
    show the fault (no partial tile, no self-pair)."""
    Z, yf = R.features(emb, pairs), np.asarray(y, dtype=np.float64)
    M = len(Z)
    if fault == "last_block_partial_dropped":
        keep = np.arange(M) < (M - 1) // rows_per_block * rows_per_block
        if not keep.any():
            return None
        Z, yf = Z[keep], yf[keep]
    elif fault == "tail_rows_dropped":
        keep = np.arange(M) < M // rows_per_block * rows_per_block
        if keep.all() or not keep.any():
            return None
        Z, yf = Z[keep], yf[keep]
    elif fault == "label_flipped":
        yf = yf.copy()
        yf[M // 2] = 1 - yf[M // 2]
    elif fault == "self_pair_as_zero":
        same = np.asarray(pairs)[:, 0] == np.asarray(pairs)[:, 1]
        if not same.any():
            return None
        Z = Z.copy()
        Z[same, :-1] = 0
    if fault == "intercept_penalised":
        with _ridge_everywhere():
            s = R.newton_step(Z, yf, theta, C, tol)
    else:
        s = R.newton_step(Z, yf, theta, C, tol)
    out = {"g": s["g"].copy(), "f0": s["f0"], "theta": s["theta"]}
    if fault == "last_column_dropped":      # g and H lose the intercept's row: the pivot is 0 and nothing moves
        out["g"][-1] = 0.0
        out["theta"] = s["theta0"]
    if fault == "rung_off_by_one" and s["k"] is not None and s["k"] < R.RUNGS - 1:
        out["theta"] = s["theta0"] - R.LADDER[s["k"] + 1] * s["d"]
    return out


def fault_factor(emb, pairs, y, theta, fault, rows_per_block, C=1.0, tol=1e-8):
    """How far outside step_bounds the faulty step lands: the largest |faulty − clean| / bound over g, f and θ."""
    Z, yf = R.features(emb, pairs), np.asarray(y, dtype=np.float64)
    ref = R.newton_step(Z, yf, theta, C, tol)
    b = step_bounds(Z, yf, ref, C)
    bad = faulty_step(emb, pairs, y, theta, fault, rows_per_block, C, tol)
    if bad is None:
        return 0.0
    t = ref["t"]
    return max(float(np.max(np.abs(bad["g"] - ref["g"]) / b["g"])), abs(bad["f0"] - ref["f0"]) / b["f0"],
               float(np.max(np.abs(bad["theta"] - ref["theta"]) / (t * b["d"] + 2 * U * np.abs(ref["theta"])))))
