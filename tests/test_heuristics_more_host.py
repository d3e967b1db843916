"""CPU checks of the RA / Jaccard / PA / Katz restatement (tests/heuristics_more_reference.py): against the plain
definitions (dense A, matrix_power, Python sets), under random summation orders against the bounds the GPU test
uses, the named faults against the same bounds, the argument checks that refuse before any GPU work, and the
public surface (header, symbol table, methods, names).

Bounds.  Local indices: exact where every term is an integer, otherwise 1 fp32 ulp + 1e-13·Σ|term| (DESIGN.md §11's
bound).  Katz, per score: 1 fp32 ulp of the restatement + 2·max_len·(m + 3)·2⁻⁵³·KATZ_{|A|,|β|}(s, d), m the largest
stored-entry count of a column: the first-order worst case of max_len dot products of at most m terms, each
followed by one add and one multiply, doubled for the higher-order terms (`M.katz_noise`, `M.katz_bound`)."""
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as ssp

import heuristics_cases as K
import heuristics_more_reference as M

REPO = Path(__file__).resolve().parent.parent
VALUE_SETS = ("A_int", "A_float", "A_signed")
KATZ_RUNS = ((0.005, 3), (0.5, 7), (-0.5, 4), (1.0, 2))
SINK_NS = (1, 15, 17, 49)
ORDERS = 8


@lru_cache(maxsize=None)
def _graphs():
    """{name: (A, links)}: the comb's three value sets, four sink graphs and a small star"""
    c = K.comb_graph()
    out = {v: (getattr(c, v), c.links) for v in VALUE_SETS}
    for n in SINK_NS:
        g = K.sink_graph(n)
        out[f"sink{n}"] = (g.A, K.links_of(K.sink_sources(g), n))
    star = K.star(9)
    out["star9"] = (star, np.stack(np.meshgrid(np.arange(10), np.arange(10))).reshape(2, -1))
    return out


def _dense(A):
    return np.asarray(M.canonical(A).todense(), dtype=np.float64)


# ---- the restatement against the definitions ----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(VALUE_SETS) + [f"sink{n}" for n in SINK_NS] + ["star9"])
def test_local_indices_equal_the_definitions(name):
    A, links = _graphs()[name]
    D = _dense(A)
    r, c = D.sum(axis=1), D.sum(axis=0)
    ar = np.abs(D).sum(axis=1)
    ra, mag = M.ra(A, links, with_magnitude=True, dtype=np.float64)
    jac, pa = M.jaccard(A, links, dtype=np.float64), M.pa(A, links, dtype=np.float64)
    if name == "A_signed":
        cols = K.comb_graph().columns
        assert np.all(c[cols["zero"]] == 0) and np.all(c[cols["negative"]] == -2)
    for l, (s, d) in enumerate(links.T):
        ks, kd = set(np.nonzero(D[s])[0]), set(np.nonzero(D[d])[0])
        terms = [D[s, k] * D[d, k] / c[k] for k in sorted(ks & kd) if c[k] != 0]
        assert abs(ra[l] - sum(terms)) <= 1e-13 * sum(abs(t) for t in terms) + 1e-300, (name, s, d)
        assert abs(mag[l] - sum(abs(t) for t in terms)) <= 1e-13 * mag[l], (name, s, d)
        either = len(ks | kd)
        assert jac[l] == (len(ks & kd) / either if either else 0.0), (name, s, d)
        assert abs(pa[l] - r[s] * r[d]) <= 1e-13 * ar[s] * ar[d], (name, s, d)   # row sums in another order
        if s == d:
            assert jac[l] == (1.0 if ks else 0.0)
    assert np.isfinite(ra).all()                                 # there is no NaN rule: nothing is NaN
    if name == "A_int":
        assert np.array_equal(pa, r[links[0]] * r[links[1]])


@pytest.mark.parametrize("name", list(VALUE_SETS) + [f"sink{n}" for n in SINK_NS] + ["star9"])
def test_katz_equals_the_sum_of_matrix_powers(name):
    """Dense powers associate and round differently: each of the max_len dense products of n-term rows adds at most
    n·2⁻⁵³ of the magnitude, so the comparison allows max_len·n·2⁻⁵²·KATZ_{|A|,|β|}."""
    A, links = _graphs()[name]
    D = _dense(A)
    n = D.shape[0]
    for beta, max_len in KATZ_RUNS:
        want = sum(beta ** l * np.linalg.matrix_power(D, l) for l in range(1, max_len + 1))
        mag = sum(abs(beta) ** l * np.linalg.matrix_power(np.abs(D), l) for l in range(1, max_len + 1))
        got = M.katz(A, links, beta, max_len, dtype=np.float64)
        err = np.abs(got - want[links[0], links[1]])
        assert np.all(err <= max_len * n * 2.0 ** -52 * mag[links[0], links[1]]), (name, beta, max_len, err.max())
        assert np.all(got[mag[links[0], links[1]] == 0] == 0)
        noise = M.katz_noise(A, links, beta, max_len)            # its magnitude is the definition's
        scale = 2.0 * max_len * (M.max_column_entries(A) + 3) * 2.0 ** -53
        assert np.allclose(noise, scale * mag[links[0], links[1]], rtol=1e-10, atol=0)


def test_katz_by_hand():
    # 0 -> 1 (2), 1 -> 2 (3), 0 -> 2 (0.5), 2 -> 0 (1): directed
    A = ssp.csr_matrix(([2.0, 0.5, 3.0, 1.0], ([0, 0, 1, 2], [1, 2, 2, 0])), shape=(3, 3))
    b = 0.25
    links = np.array([[0, 0, 2, 1, 0], [2, 0, 1, 0, 1]])
    # walks 0 -> 2: length 1 (0.5), 2 via 1 (6), 3 round the cycle 0-2-0-2 (0.25); 0 -> 0: length 2 (0.5), 3 (6);
    # 2 -> 1: length 2 (2); 1 -> 0: length 2 (3); 0 -> 1: length 1 (2), 3 as 0-2-0-1 (1)
    want = [b * 0.5 + b * b * 6 + b ** 3 * 0.25, b * b * 0.5 + b ** 3 * 6, b * b * 2, b * b * 3, b * 2 + b ** 3]
    assert np.array_equal(M.katz(A, links, b, 3, dtype=np.float64), np.array(want))
    assert np.array_equal(M.katz(A, links[:, :1], b, 1, dtype=np.float64), [b * 0.5])


# ---- random summation orders against the bounds -------------------------------------------------------------------

def _dyadic(beta):
    return float(beta * 8).is_integer()


@pytest.mark.parametrize("values", VALUE_SETS)
def test_katz_under_random_orders_stays_within_half_the_bound(values):
    A, links = _graphs()[values]
    worst = 0.0
    for beta, max_len in KATZ_RUNS:
        fwd = M.katz(A, links, beta, max_len, dtype=np.float64)
        noise = M.katz_noise(A, links, beta, max_len)
        for seed in range(ORDERS):
            got = M.katz(A, links, beta, max_len, sums=M.Sums(np.random.default_rng(seed)), dtype=np.float64)
            if values == "A_int" and _dyadic(beta):
                assert np.array_equal(got, fwd), (beta, max_len, seed)
                continue
            err = np.abs(got - fwd)
            assert np.all(err <= 0.5 * noise), (values, beta, max_len, seed)
            assert np.all(got[noise == 0] == 0)
            worst = max(worst, float(np.max(err[noise > 0] / noise[noise > 0])))
    print(f"[heuristics more] Katz {values}: random orders reach {worst:.4f} of the bound's fp64 part")


@pytest.mark.parametrize("values", VALUE_SETS)
def test_local_indices_under_random_orders(values):
    A, links = _graphs()[values]
    ra, mag = M.ra(A, links, with_magnitude=True, dtype=np.float64)
    jac, pa = M.jaccard(A, links, dtype=np.float64), M.pa(A, links, dtype=np.float64)
    for seed in range(ORDERS):
        sums = M.Sums(np.random.default_rng(seed))
        assert np.array_equal(M.jaccard(A, links, sums=sums, dtype=np.float64), jac)
        got_pa = M.pa(A, links, sums=sums, dtype=np.float64)
        got_ra = M.ra(A, links, sums=sums, dtype=np.float64)
        if values != "A_float":                                  # integer row sums: exact in any order
            assert np.array_equal(got_pa, pa)
        assert np.all(np.abs(got_pa - pa) <= 1e-13 * np.abs(pa))
        assert np.all(np.abs(got_ra - ra) <= 1e-13 * mag)


def test_sums_with_an_rng_really_reorder():
    A = K.comb_graph().A_float
    T = M.Sums(np.random.default_rng(0)).ordered(A)
    assert not np.array_equal(T.indices, A.indices) and (T != A).nnz == 0
    assert np.array_equal(M.Sums().ordered(A).indices, A.indices)


# ---- the named faults leave the bounds ----------------------------------------------------------------------------

def _local_excess(A, links, fault):
    """the largest |fault − restatement| / bound over RA, Jaccard and PA"""
    ra, mag = M.ra(A, links, with_magnitude=True)
    worst = 0.0
    for ref, bad, noise in ((ra, M.ra(A, links, fault=fault), 1e-13 * mag),
                            (M.jaccard(A, links), M.jaccard(A, links, fault=fault), 0.0),
                            (M.pa(A, links), M.pa(A, links, fault=fault), 0.0)):
        if not np.isfinite(bad).all():
            return np.inf
        err = np.abs(bad.astype(np.float64) - ref.astype(np.float64))
        worst = max(worst, float(np.max(err / (M.ulp32(ref) + noise))))
    return worst


def _katz_excess(A, links, fault):
    worst = 0.0
    for beta, max_len in KATZ_RUNS:
        ref = M.katz(A, links, beta, max_len)
        bad = M.katz(A, links, beta, max_len, fault=fault)
        err = np.abs(bad.astype(np.float64) - ref.astype(np.float64))
        worst = max(worst, float(np.max(err / M.katz_bound(A, links, beta, max_len))))
    return worst


@pytest.mark.parametrize("fault", M.FAULTS)
def test_every_fault_lands_ten_times_outside_the_bounds(fault):
    katz = fault.startswith("katz") or fault == "finish_reads_buffer_0"
    names = [f"sink{n}" for n in (15, 17, 49)] + list(VALUE_SETS)
    excess = {name: (_katz_excess if katz else _local_excess)(*_graphs()[name], fault) for name in names}
    print(f"[heuristics more] fault {fault}: error / bound at worst {excess}")
    assert max(excess.values()) >= 10.0
    if fault == "katz_no_transpose":                            # the directed sink graphs catch it
        assert all(excess[f"sink{n}"] >= 10.0 for n in (15, 17, 49))


def test_the_faultless_restatement_is_inside_its_own_bounds():
    for name, (A, links) in _graphs().items():
        assert _local_excess(A, links, None) == 0.0 and _katz_excess(A, links, None) == 0.0, name


# ---- argument checks, before any GPU work -------------------------------------------------------------------------

def _shell():
    """a Heuristics that never touched the GPU: its argument checks run before anything else"""
    from s3grl_amd.heuristics import Heuristics

    h = Heuristics.__new__(Heuristics)
    h.num_nodes, h._h = 3, None
    return h


@pytest.mark.parametrize("kw", [dict(beta=float("nan")), dict(beta=float("inf")), dict(beta=-float("inf")),
                                dict(max_len=0), dict(max_len=65), dict(max_len=2.5), dict(block_width=96),
                                dict(block_width=2048), dict(block_width=32)])
def test_katz_refuses_arguments_outside_the_envelope(kw):
    from s3grl_amd import heuristics as H
    from s3grl_amd.recommend import HeuristicScorer

    A = ssp.csr_matrix(([1, 1], ([0, 1], [1, 0])), shape=(3, 3))
    ei = np.array([[0, 1], [1, 2]])
    with pytest.raises(ValueError):
        H.check_katz(**{"beta": 0.005, "max_len": 3, **kw})
    with pytest.raises(ValueError):
        _shell().katz(ei, **kw)
    with pytest.raises(ValueError):
        H.run_heuristic(None, "KATZ", **kw)
    with pytest.raises(ValueError):
        HeuristicScorer(None, "KATZ", **kw)
    if "block_width" not in kw:
        with pytest.raises(ValueError):
            H.Katz(A, ei, **kw)


def test_the_envelope_itself_is_accepted():
    from s3grl_amd import heuristics as H

    assert H.check_katz(0.005, 3) == (0.005, 3, 0)
    assert H.check_katz(-1e300, 64, 1024) == (-1e300, 64, 1024)
    assert H.check_katz(0, np.int64(1), 64) == (0.0, 1, 64)


def test_bad_ids_raise_before_any_gpu_work():
    from s3grl_amd import heuristics as H

    A = ssp.csr_matrix(([1, 1], ([0, 1], [1, 0])), shape=(3, 3))
    for bad in ([[0, 3], [1, 0]], [[0, -1], [1, 2]], [[0, 1, 2]]):
        ei = np.array(bad)
        for fn in (H.RA, H.Jaccard, H.PA, H.Katz):
            with pytest.raises(ValueError):
                fn(A, ei)
        with pytest.raises(ValueError):
            _shell().katz(ei)
    with pytest.raises(RuntimeError):                            # good arguments reach the closed object
        _shell().katz(np.array([[0], [1]]))


def test_unknown_names_keep_their_errors():
    from s3grl_amd import heuristics as H
    from s3grl_amd.recommend import HeuristicScorer

    for name in ("SALTON", "", "KATZ2"):
        with pytest.raises(ValueError, match="unknown heuristic"):
            H.run_heuristic(None, name)
    for kind in ("PPR", "ra", "SALTON", None):
        with pytest.raises(ValueError, match="kind"):
            HeuristicScorer(None, kind)
    with pytest.raises(ValueError):
        HeuristicScorer(None, "RA", beta=0.1)                    # only KATZ takes keyword arguments
    with pytest.raises(ValueError):
        HeuristicScorer(None, "KATZ", tol=0.1)
    for kind in ("CN", "AA", "RA", "JACCARD", "PA", "KATZ"):
        assert HeuristicScorer(None, kind).kind == kind
    assert HeuristicScorer(None, "KATZ", beta=0.1, max_len=5).kw == dict(beta=0.1, max_len=5)


# ---- the public surface: fails without the feature ----------------------------------------------------------------

def test_the_four_indices_are_declared_exported_and_named():
    from s3grl_amd import _native
    from s3grl_amd import heuristics as H

    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_heuristics_[a-z_]+)\s*\(", header))
    assert declared == {"s3grl_heuristics_create", "s3grl_heuristics_pairs", "s3grl_heuristics_ppr",
                        "s3grl_heuristics_katz", "s3grl_heuristics_destroy"}
    assert declared <= set(_native.SYMBOLS)
    for kind, value in (("CN", 0), ("AA", 1), ("RA", 2), ("JACCARD", 3), ("PA", 4)):
        assert re.search(rf"#define\s+S3GRL_HEURISTIC_{kind}\s+{value}\b", header) and H.KIND[kind] == value
    lib = _native.lib()
    assert getattr(lib, "s3grl_heuristics_katz") is not None and lib.s3grl_abi_version() == 6
    for method in ("ra", "jaccard", "pa", "katz", "cn", "aa", "ppr"):
        assert callable(getattr(H.Heuristics, method))
    assert H.NAMES[:3] == ("CN", "AA", "PPR") and set(H.NAMES[3:]) == {"RA", "JACCARD", "PA", "KATZ"}
    for twin in ("RA", "Jaccard", "PA", "Katz"):
        assert callable(getattr(H, twin))
    # through the C ABI: refusals that need no object and no GPU
    null = None
    assert lib.s3grl_heuristics_katz(null, null, 0, null, 0, 0.005, 3, 0, null) != 0
    assert lib.s3grl_heuristics_pairs(null, 2, null, 0, null) != 0
