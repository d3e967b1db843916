"""The link metrics without a GPU: the numpy restatement against sklearn and hand-worked cases, the exact-integer AUC
against the trapezoid, the kernels' layout, the C ABI's new symbols, and every argument error the host can detect."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import metrics_reference as ref
from s3grl_amd import _native, metrics

REPO = Path(__file__).resolve().parent.parent
METRIC_SYMBOLS = {"s3grl_metrics_layout", "s3grl_metrics_create", "s3grl_metrics_ranked", "s3grl_metrics_mrr",
                  "s3grl_metrics_destroy"}


def _cases():
    rng = np.random.default_rng(7)
    out = {}
    y = (rng.random(501) < 0.3).astype(np.int64)
    out["untied"] = (y, rng.standard_normal(501).astype(np.float32))
    out["tied"] = (y, rng.integers(0, 6, 501).astype(np.float32))
    out["mostly_one_value"] = (y, np.where(rng.random(501) < 0.9, 0.0, rng.integers(1, 4, 501)).astype(np.float32))
    out["signed_zero"] = (np.array([1, 0, 1, 0, 0]), np.array([0.0, -0.0, 1.0, -1.0, 0.0], dtype=np.float32))
    out["inf"] = (np.array([1, 0, 1, 0, 1]), np.array([np.inf, np.inf, -np.inf, 0.0, 1e-45], dtype=np.float32))
    return out


CASES = _cases()


# ---- the restatement against sklearn ------------------------------------------------------------------------------------
FINITE = sorted(set(CASES) - {"inf"})                  # sklearn refuses infinite scores


@pytest.mark.parametrize("name", FINITE)
def test_reference_is_sklearn(name):
    skm = pytest.importorskip("sklearn.metrics")
    y, s = CASES[name]
    assert ref.roc_auc(y, s) == pytest.approx(skm.roc_auc_score(y, s), abs=1e-14)
    assert ref.average_precision(y, s) == pytest.approx(skm.average_precision_score(y, s), abs=1e-14)
    assert ref.roc_auc_exact(y, s) == pytest.approx(skm.roc_auc_score(y, s), abs=1e-14)


@pytest.mark.parametrize("name", FINITE)
def test_reference_is_the_numpy_path(name):
    from s3grl_amd import heuristics

    y, s = CASES[name]
    assert ref.roc_auc(y, s) == heuristics.roc_auc(y, s)
    assert ref.average_precision(y, s) == heuristics.average_precision(y, s)


def test_infinite_scores_are_values():
    # descending: +inf (+, −), 1e-45 (+), 0 (−), −inf (+): the two +inf are ONE threshold
    y, s = CASES["inf"]
    assert ref.thresholds(s) == 4
    assert ref.auc_numerator(y, s) == (1 * 1 + 0 + 1 * 4 + 0, 3, 2)
    assert ref.roc_auc(y, s) == pytest.approx(5 / 12, abs=1e-15)
    assert ref.average_precision(y, s) == pytest.approx((1 / 3) * (1 / 2) + (1 / 3) * (2 / 3) + (1 / 3) * (3 / 5), abs=1e-15)


@pytest.mark.parametrize("name", sorted(CASES))
def test_exact_integer_auc_is_the_trapezoid(name):
    y, s = CASES[name]
    num, P, Nn = ref.auc_numerator(y, s)
    assert (P, Nn) == (int(np.sum(y == 1)), int(np.sum(y == 0)))
    assert 0 <= num <= 2 * P * Nn
    # one rounding in the quotient against a trapezoid of at most 501 rounded terms
    assert num / (2 * P * Nn) == pytest.approx(ref.roc_auc(y, s), abs=501 * 2.0 ** -53)


def test_auc_numerator_by_hand():
    # descending: 3 (+), 2 (+, −), 1 (−): groups (tp_b, tp_g, fp_g) = (0, 1, 0), (1, 1, 1), (2, 0, 1)
    y, s = [1, 1, 0, 0], [3.0, 2.0, 2.0, 1.0]
    assert ref.auc_numerator(y, s) == (0 * 1 + 1 * 3 + 1 * 4, 2, 2)
    assert ref.roc_auc_exact(y, s) == 7 / 8
    assert ref.thresholds(s) == 3
    assert ref.thresholds([0.0, -0.0, np.inf, np.inf, -np.inf]) == 3


def test_hits_by_hand():
    pos, neg = [0.9, 0.5, 0.5, 0.1], [0.8, 0.5, 0.3]
    assert ref.hits_at(pos, neg, 1) == 1 / 4         # above 0.8
    assert ref.hits_at(pos, neg, 2) == 1 / 4         # the 2nd negative ties two positives: they do not count
    assert ref.hits_at(pos, neg, 3) == 3 / 4         # above 0.3
    assert ref.hits_at(pos, neg, 4) == 1.0           # fewer than K negatives
    assert ref.hits_count(pos, neg, 4) is None


def test_mrr_by_hand():
    pos = [0.5, 0.5, 0.5, 0.5]
    neg = [[0.1, 0.2, 0.3], [0.5, 0.2, 0.3], [0.9, 0.5, 0.5], [0.9, 0.9, 0.9]]
    lst, rank = ref.mrr_list(pos, neg)
    assert rank.tolist() == [1.0, 1.5, 3.0, 4.0]     # a tie with one negative: rank 1.5
    assert lst.dtype == np.float32
    assert lst.tolist() == [1.0, np.float32(1) / np.float32(1.5), np.float32(1) / np.float32(3), 0.25]
    r = ref.mrr(pos, neg)
    assert r["hits@1"] == 0.25 and r["hits@3"] == 0.75 and r["hits@10"] == 1.0
    assert r["MRR"] == pytest.approx((1 + 1 / 1.5 + 1 / 3 + 0.25) / 4, abs=1e-7)


def test_mrr_without_ties_is_the_argsort_form():
    rng = np.random.default_rng(3)
    pos, neg = rng.standard_normal(40).astype(np.float32), rng.standard_normal((40, 17)).astype(np.float32)
    both = np.concatenate([pos[:, None], neg], axis=1)
    rank = np.nonzero(np.argsort(-both, axis=1) == 0)[1] + 1
    assert ref.mrr_list(pos, neg)[1].tolist() == rank.astype(np.float32).tolist()


# ---- layout and ABI -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 1025, (1 << 31) - 1])
def test_layout_is_sane(M):
    lay = metrics.layout(M)
    T, v = lay["block_items"], lay["vector_width"]
    assert T >= 64 and T % 64 == 0
    assert v == 4                                            # 16-byte loads of fp32
    assert lay["rows_per_wave"] * lay["lanes_per_row"] == 64
    assert lay["rows_per_block"] % lay["rows_per_wave"] == 0
    lanes = lay["lanes_per_row"]
    assert lanes & (lanes - 1) == 0
    need = -(-M // v)                                        # vector loads that cover a row
    assert lanes == 64 or lanes >= need                      # one load per lane covers a short row ...
    assert lanes == 1 or lanes < 2 * need                    # ... with no more than half the lanes idle
    assert lay["max_ks"] >= 3


def test_layout_rejects_bad_rows():
    for M in (0, -1, 1 << 31):
        with pytest.raises(ValueError):
            metrics.layout(M)


def test_symbols_declared_and_exported():
    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_metrics_[a-z_]+)\s*\(", header))
    assert declared == METRIC_SYMBOLS
    assert METRIC_SYMBOLS <= set(_native.SYMBOLS)
    lib = _native.lib()
    for name in METRIC_SYMBOLS:
        assert getattr(lib, name).argtypes is not None
    assert _native.ABI_VERSION == 6 and lib.s3grl_abi_version() == 6
    assert "s3grl_metrics.hip" in __import__("__graft_entry__").SOURCES
    assert callable(__import__("s3grl_amd").LinkMetrics)
    assert re.search(r"#define S3GRL_ABI_VERSION 6\b", header)


# ---- argument errors, all raised before a device is asked for ------------------------------------------------------------
GOOD = (torch.tensor([0.3, 0.1, 0.7]), torch.tensor([1, 0, 1]))


def test_cpu_device_is_refused():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.LinkMetrics(device="cpu")


@pytest.mark.parametrize("pred, true", [
    (torch.tensor([0.3, 0.1]), torch.tensor([1, 1])),                    # AUC without a negative
    (torch.tensor([0.3, 0.1]), torch.tensor([0, 0])),                    # AP without a positive
    (torch.tensor([0.3, 0.1, 0.2]), torch.tensor([1, 0])),               # lengths
    (torch.tensor([0.3, 0.1]), torch.tensor([1, 2])),                    # a label outside {0, 1}
    (torch.tensor([0.3, 0.1]), torch.tensor([1.0, 0.5])),
    (torch.tensor([0.3, float("nan")]), torch.tensor([1, 0])),           # NaN
    (torch.tensor([]), torch.tensor([])),
    (np.array([0.3, 0.1]), np.array([True, True])),
])
def test_evaluate_auc_errors(pred, true):
    with pytest.raises(ValueError):
        metrics.evaluate_auc(pred, true, *GOOD)
    with pytest.raises(ValueError):
        metrics.evaluate_auc(*GOOD, pred, true)


def test_evaluate_hits_and_rocauc_errors():
    pos, neg = torch.tensor([0.5, 0.2]), torch.tensor([0.1, 0.3, 0.4])
    none = torch.tensor([])
    with pytest.raises(ValueError):
        metrics.evaluate_hits(none, neg, pos, neg)                       # Hits without a positive
    with pytest.raises(ValueError):
        metrics.evaluate_hits(pos, neg, pos, torch.tensor([0.1, float("nan")]))
    with pytest.raises(ValueError):
        metrics.evaluate_ogb_rocauc(pos, none, pos, neg)                 # AUC without a negative
    with pytest.raises(ValueError):
        metrics.evaluate_ogb_rocauc(pos, neg, none, neg)


def test_evaluate_mrr_errors():
    pos = torch.tensor([0.5, 0.2, 0.1])
    ok = torch.zeros(6)
    with pytest.raises(ValueError):
        metrics.evaluate_mrr(pos, torch.zeros(7), pos, ok)               # P · M not divisible by P
    with pytest.raises(ValueError):
        metrics.evaluate_mrr(pos, ok, pos, torch.zeros(2, 3))            # rows are not the positives
    with pytest.raises(ValueError):
        metrics.evaluate_mrr(torch.tensor([]), ok, pos, ok)              # MRR without a positive
    with pytest.raises(ValueError):
        metrics.evaluate_mrr(pos, torch.zeros(0), pos, ok)               # no negatives at all
    with pytest.raises(ValueError):
        metrics.evaluate_mrr(pos, ok, pos, torch.full((6,), float("nan")))


def test_k_values_are_checked():
    for ks in ((0,), (-3,), (20, 20)):
        with pytest.raises(ValueError):
            metrics._ranked_args(*GOOD, ks)


def test_fit_and_select_checks_its_metric():
    from s3grl_amd import harness

    with pytest.raises(ValueError, match="eval_metric"):
        harness.fit_and_select(None, None, None, eval_metric="f1")
