"""Host checks of the side-by-side SIGNNet runs (no GPU): the group call is part of the ABI, its argument checks that
need no device (C and Python), and `harness.run_statistics` against a restatement of the reference Logger's summary
(utils.py:769-792) written here with torch.tensor(..).mean() / .std()."""
import ctypes as C
import math
import re
from pathlib import Path

import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def signnet():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd import signnet as module

    return module


# ---- the ABI -------------------------------------------------------------------------------------------------------
def test_the_group_call_is_part_of_the_abi(signnet):
    import s3grl_amd
    from s3grl_amd import _native, harness

    header = (REPO / "include" / "s3grl.h").read_text()
    assert re.search(r"\bs3grl_status\s+s3grl_signnetruns_fit_epoch\s*\(\s*s3grl_signnet\s*\*\s*const\s*\*\s*members,"
                     r"\s*int32_t\s+num_members,\s*int64_t\s+epoch,", header)
    assert "s3grl_signnetruns_fit_epoch" in _native.SYMBOLS
    fn = _native.lib().s3grl_signnetruns_fit_epoch
    assert len(fn.argtypes) == 11
    assert _native.SIGNNET_MAX_RUNS == 16
    assert callable(s3grl_amd.SIGNNetRuns) and callable(harness.fit_and_select_runs) and callable(harness.run_statistics)


def test_the_c_call_rejects_bad_arguments_before_any_device_work(signnet):
    from s3grl_amd import _native as N

    fn = N.lib().s3grl_signnetruns_fit_epoch
    lr = (C.c_double * 17)(*([1e-3] * 17))
    some = C.c_void_p(64)                      # never dereferenced: every call below fails before that

    def call(members, n, rates, rows=some):
        return fn(members, n, 0, rows, 10, some, some, 4, 2, rates, None)

    nulls = (C.c_void_p * 17)()                # 17 null handles
    assert call(None, 1, lr) == N.ERR_INVALID_ARGUMENT
    assert call(nulls, 0, lr) == N.ERR_INVALID_ARGUMENT
    assert call(nulls, -1, lr) == N.ERR_INVALID_ARGUMENT
    assert call(nulls, 1, None) == N.ERR_INVALID_ARGUMENT
    assert call(nulls, 17, lr) == N.ERR_NOT_IMPLEMENTED
    assert "16" in N.lib().s3grl_last_error().decode()      # the message names the limit
    with pytest.raises(NotImplementedError, match="16"):
        N.check(call(nulls, 17, lr), "s3grl_signnetruns_fit_epoch")
    assert call(nulls, 16, lr) == N.ERR_INVALID_ARGUMENT    # a null handle
    assert call(nulls, 1, lr, rows=None) == N.ERR_INVALID_ARGUMENT


def test_python_argument_checks(signnet):
    T = signnet.SIGNNetRuns
    with pytest.raises(ValueError, match="one run or more"):
        T(12, 8, seeds=())
    with pytest.raises(NotImplementedError, match="16"):
        T(12, 8, seeds=range(17))
    with pytest.raises(ValueError, match="dropout"):
        T(12, 8, dropout=(0.5, 0.5), seeds=(1, 2, 3))
    with pytest.raises(ValueError, match="lr"):
        T(12, 8, lr=(1e-3,), seeds=(1, 2))
    with pytest.raises(ValueError, match="dropout"):
        T(12, 8, dropout=(1.0, 0.5), seeds=(1, 2), device="cpu")      # the member's own check
    with pytest.raises(NotImplementedError, match="concat"):
        T(12, 8, k_heuristic=2, k_pool_strategy="concat", seeds=(1,))
    with pytest.raises(NotImplementedError, match="256"):
        T(12, 257, seeds=(1,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T(12, 8, seeds=(1, 2), device="cpu")
    from s3grl_amd import harness

    store = (torch.zeros(4, 2, 3), torch.tensor([0, 2, 4]), torch.tensor([1.0, 0.0]))
    with pytest.raises(ValueError, match="eval_metric"):
        harness.fit_and_select_runs(store, store, store, eval_metric="f1")
    with pytest.raises(ValueError, match="one epoch"):
        harness.fit_and_select_runs(store, store, store, epochs=0)
    with pytest.raises(ValueError, match="one run"):
        harness.fit_and_select_runs(store, store, store, runs=0)
    with pytest.raises(NotImplementedError, match="16"):
        harness.fit_and_select_runs(store, store, store, runs=17)


# ---- run_statistics ------------------------------------------------------------------------------------------------
# 3 runs × 4 epochs of (valid, test).  Run 0 ties in the valid column at epochs 1 and 3 (the first wins: test 0.61, not
# 0.70); run 1 peaks at its last epoch; run 2 at its first.
HISTORY = [
    [(0.50, 0.40), (0.80, 0.61), (0.70, 0.65), (0.80, 0.70)],
    [(0.55, 0.45), (0.60, 0.50), (0.65, 0.55), (0.90, 0.72)],
    [(0.85, 0.66), (0.60, 0.69), (0.84, 0.71), (0.10, 0.05)],
]


def logger_summary(runs):
    """The reference Logger's all-runs summary of [[(valid, test) per epoch] per run], restated."""
    result = 100 * torch.tensor(runs)
    best = []
    for r in result:
        col = r[:, 0].tolist()
        first = col.index(max(col))
        best.append((r[first, 0].item(), r[first, 1].item(), first))
    valid, test = torch.tensor([b[0] for b in best]), torch.tensor([b[1] for b in best])
    every = result[:, :, 1].reshape(-1)
    return best, valid, test, every


def _eq(got, want):
    return (math.isnan(got) and math.isnan(want)) or got == want


def test_run_statistics_is_the_loggers_summary(signnet):
    from s3grl_amd.harness import run_statistics

    other = [[(v / 2, t / 3) for v, t in run] for run in HISTORY]
    stats = run_statistics([{"AUC": a, "AP": b} for a, b in zip(HISTORY, other)])
    assert set(stats) == {"AUC", "AP"}
    for key, runs in (("AUC", HISTORY), ("AP", other)):
        best, valid, test, every = logger_summary(runs)
        s = stats[key]
        assert [(p["highest_valid"], p["highest_test"], p["best_epoch"]) for p in s["per_run"]] == best
        assert s["highest_valid"] == {"mean": valid.mean().item(), "std": valid.std().item()}
        assert s["highest_test"] == {"mean": test.mean().item(), "std": test.std().item()}
        assert s["average_test"] == {"mean": every.mean().item(), "std": every.std().item()}
        assert s["highest_test_5"] == f"{test.mean():.5f} ± {test.std():.5f}"
    # the tie: the first of the two epochs with valid 0.80
    assert stats["AUC"]["per_run"][0]["best_epoch"] == 1
    assert stats["AUC"]["per_run"][0]["highest_test"] == (100 * torch.tensor(0.61)).item()
    assert [p["best_epoch"] for p in stats["AUC"]["per_run"]] == [1, 3, 0]
    # unbiased: three values 61, 72, 66 have std sqrt(30.33..)
    assert abs(stats["AUC"]["highest_test"]["std"] - math.sqrt(((61 - 199 / 3) ** 2 + (72 - 199 / 3) ** 2 +
                                                                (66 - 199 / 3) ** 2) / 2)) < 1e-4
    assert abs(stats["AUC"]["highest_test"]["mean"] - 199 / 3) < 1e-4


def test_run_statistics_of_one_run_has_nan_std(signnet):
    from s3grl_amd.harness import run_statistics

    s = run_statistics([{"MRR": HISTORY[1]}])["MRR"]
    best, valid, test, every = logger_summary([HISTORY[1]])
    assert math.isnan(s["highest_valid"]["std"]) and math.isnan(s["highest_test"]["std"])
    assert s["highest_valid"]["mean"] == valid.mean().item() and s["highest_test"]["mean"] == test.mean().item()
    assert _eq(s["average_test"]["std"], every.std().item()) and not math.isnan(s["average_test"]["std"])
    assert s["highest_test_5"].endswith("± nan")
    with pytest.raises(ValueError):
        run_statistics([])
    with pytest.raises(ValueError, match="epochs"):
        run_statistics([{"MRR": HISTORY[0]}, {"MRR": HISTORY[1][:3]}])
