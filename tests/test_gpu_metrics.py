"""s3grl_amd.metrics on the MI355X against the numpy restatement (tests/metrics_reference.py).  Sizes come from
`metrics.layout`: T = block_items is the number of sorted scores one workgroup of the scan passes takes.

Tolerances (derived, not tuned):
- AUC abs <= 1e-12: the device value is an exact integer over 2PN with one rounding; the restatement's trapezoid differs
  from that by at most 1.2e-16 for n up to 2 M.
- AP abs <= 1e-11: any summation order of at most n non-negative terms that sum to at most 1 errs by at most n·2^-53,
  7e-12 at n = 65 537, the largest n compared with the restatement; the 2^24 + 3 case uses n·2^-53 against its closed form.
- P, N, thresholds and the Hits counts: equal as integers.  mrr_list: bit-equal to numpy's fp32 1 / rank.  The MRR mean:
  abs <= P·2^-53 against the fp64 mean of the list.
"""
import numpy as np
import pytest
import torch

import metrics_reference as ref

pytestmark = pytest.mark.gpu

AUC_TOL, AP_TOL = 1e-12, 1e-11


@pytest.fixture(scope="module")
def lm():
    from s3grl_amd import metrics

    m = metrics.LinkMetrics("cuda:0")
    yield m
    m.close()


@pytest.fixture(scope="module")
def T():
    from s3grl_amd import metrics

    return metrics.layout()["block_items"]


def dev(x, dtype=None):
    return torch.as_tensor(np.asarray(x), dtype=dtype).to("cuda:0")


def check_ranked(lm, s, y, ks=()):
    """One `ranked` call on device tensors against the restatement; returns the result."""
    s, y = np.asarray(s, dtype=np.float32), np.asarray(y)
    r = lm.ranked(dev(s), dev(y), ks=ks)
    num, P, Nn = ref.auc_numerator(y, s)
    print(f"n={s.size} P={P} N={Nn} thr={r['thresholds']} AUC={r['AUC']!r} ref={ref.roc_auc(y, s)!r} "
          f"AP={r['AP']!r} ref={ref.average_precision(y, s)!r} hits={r['hits']}")
    assert (r["num_pos"], r["num_neg"], r["thresholds"]) == (P, Nn, ref.thresholds(s))
    assert r["AUC"] == num / (2 * P * Nn)                     # the same exact integer, the same one division
    assert abs(r["AUC"] - ref.roc_auc(y, s)) <= AUC_TOL
    assert abs(r["AP"] - ref.average_precision(y, s)) <= AP_TOL
    pos, neg = s[y == 1], s[y == 0]
    for k in ks:
        c = ref.hits_count(pos, neg, k)
        assert r["hits"][k] == (1.0 if c is None else c / P), (k, r["hits"][k], c)
    return r


def sorted_layout(groups, rng):
    """groups: [(size, labels or None)] from the highest score down, each one tie group -> (scores, labels) shuffled.
    Labels default to random."""
    s, y = [], []
    top = float(len(groups))
    for g, (size, lab) in enumerate(groups):
        s.append(np.full(size, top - g, dtype=np.float32))
        y.append(rng.integers(0, 2, size) if lab is None else np.asarray(lab))
    s, y = np.concatenate(s), np.concatenate(y)
    y[0], y[-1] = 1, 0                                         # both classes
    p = rng.permutation(s.size)
    return s[p], y[p]


# ---- ranked ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s, y", [([0.9, 0.1], [1, 0]), ([0.1, 0.9], [1, 0]), ([0.5, 0.5], [1, 0])])
def test_two_scores(lm, s, y):
    r = check_ranked(lm, s, y, ks=(1, 2))
    assert r["AUC"] == {0.9: 1.0, 0.1: 0.0, 0.5: 0.5}[s[0]]
    assert r["hits"] == {1: 1.0 if s[0] == 0.9 else 0.0, 2: 1.0}


@pytest.mark.parametrize("off", ["T-1", "T", "T+1", "3T+5"])
@pytest.mark.parametrize("kind", ["untied", "tied"])
def test_sizes_around_a_workgroup(lm, T, off, kind):
    n = {"T-1": T - 1, "T": T, "T+1": T + 1, "3T+5": 3 * T + 5}[off]
    rng = np.random.default_rng(n)
    y = (rng.random(n) < 0.4).astype(np.int64)
    y[:2] = (1, 0)
    s = rng.standard_normal(n) if kind == "untied" else rng.integers(0, 7, n)
    Nn = int(np.sum(y == 0))
    check_ranked(lm, s, y, ks=(1, 20, Nn, Nn + 1))


def test_all_scores_equal(lm, T):
    n = 3 * T + 5
    rng = np.random.default_rng(0)
    y = (rng.random(n) < 0.3).astype(np.int64)
    y[:2] = (1, 0)
    P, Nn = int(y.sum()), int(n - y.sum())
    r = check_ranked(lm, np.full(n, 2.5), y, ks=(1, Nn, Nn + 1))
    assert r["thresholds"] == 1
    assert r["AUC"] == 0.5 and r["AP"] == P / n
    assert r["hits"] == {1: 0.0, Nn: 0.0, Nn + 1: 1.0}


def test_tie_group_over_three_workgroups(lm, T):
    # sorted positions: T − 1 singletons, then ONE group on positions T − 1 .. 2T (the last element of workgroup 0, all
    # of workgroup 1, the first element of workgroup 2), then singletons
    rng = np.random.default_rng(1)
    groups = [(1, None)] * (T - 1) + [(T + 2, None)] + [(1, None)] * (T + 3)
    s, y = sorted_layout(groups, rng)
    assert s.size == 3 * T + 4
    r = check_ranked(lm, s, y, ks=(1, T // 2, T, 3 * T // 2))
    assert r["thresholds"] == len(groups)


def test_group_ends_on_a_workgroups_last_element(lm, T):
    rng = np.random.default_rng(2)
    groups = [(1, None)] * (T - 5) + [(5, None)] + [(1, None)] * 7 + [(2 * T - 7, None)] + [(3, None)]
    s, y = sorted_layout(groups, rng)          # groups end on positions T − 1 and 3T − 1
    check_ranked(lm, s, y, ks=(1, 5, T))


def test_signed_zeros_are_one_threshold(lm):
    s = np.array([0.0, -0.0, 1.0, -1.0, 0.0, -0.0], dtype=np.float32)
    r = check_ranked(lm, s, [1, 0, 1, 0, 0, 1], ks=(1, 2, 3))
    assert r["thresholds"] == 3


def test_special_values(lm):
    tiny = np.float32(1e-45)                                   # the smallest denormal
    one = np.float32(1.0)
    s = np.array([np.inf, np.inf, -np.inf, -np.inf, tiny, -tiny, 0.0, 2 * tiny, one, np.nextafter(one, np.float32(2)),
                  np.nextafter(one, np.float32(0)), -one, np.nextafter(-one, np.float32(-2)), -3.5, 3.4e38, -3.4e38],
                 dtype=np.float32)
    y = np.array([1, 0, 1, 0, 1, 0, 0, 1, 0, 1, 1, 0, 1, 0, 1, 0])
    r = check_ranked(lm, s, y, ks=(1, 2, 3, 8))
    assert r["thresholds"] == 14                               # the infinities pair up
    check_ranked(lm, s, 1 - y, ks=(1, 2, 3, 8))


def test_common_neighbour_like_scores(lm):
    n = 65537
    rng = np.random.default_rng(5)
    y = (np.arange(n) % 11 == 0).astype(np.int64)              # 1 : 10
    s = np.where(rng.random(n) < 0.85, 0, rng.poisson(2.0, n)) + 3 * y * (rng.random(n) < 0.5)
    check_ranked(lm, s, y, ks=(20, 50, 100))


def test_k_at_the_edges_and_a_tied_kth_negative(lm):
    # descending: 9 (+), 7 (+ + −), 5 (−), 3 (+ −): the 1st negative ties two positives, which do not count
    s = [9, 7, 7, 7, 5, 3, 3]
    y = [1, 1, 1, 0, 0, 1, 0]
    r = check_ranked(lm, s, y, ks=(1, 2, 3, 4))
    assert r["hits"] == {1: 1 / 4, 2: 3 / 4, 3: 3 / 4, 4: 1.0}   # K = N = 3 and K = N + 1 = 4


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.bool, torch.uint8, torch.float32, torch.float64])
def test_label_dtypes_and_the_n_pos_form(lm, T, dtype):
    n, P = T + 37, 301
    rng = np.random.default_rng(6)
    s = np.round(rng.standard_normal(n), 1).astype(np.float32)
    y = np.r_[np.ones(P, dtype=np.int64), np.zeros(n - P, dtype=np.int64)]
    a = lm.ranked(dev(s), dev(y).to(dtype), ks=(20, 50))
    b = lm.ranked(dev(s), n_pos=P, ks=(20, 50))
    c = lm.ranked(s, y.astype(bool), ks=(20, 50))              # host arrays are uploaded
    assert a == b == c
    assert a["AUC"] == ref.roc_auc_exact(y, s)
    assert lm.hits(dev(s[:P]), dev(s[P:]), ks=(20, 50)) == a["hits"]
    assert lm.rocauc(dev(s[:P]), dev(s[P:])) == a["AUC"]


def test_unaligned_scores(lm, T):
    n = T + 3
    rng = np.random.default_rng(8)
    buf, y = dev(rng.integers(0, 9, n + 1), torch.float32), (rng.random(n) < 0.5).astype(np.int64)
    y[:2] = (1, 0)
    r = lm.ranked(buf[1:], dev(y)[0:], ks=(3,))                 # 4 bytes past a 16-byte boundary
    s = buf[1:].cpu().numpy()
    assert r["AUC"] == ref.roc_auc_exact(y, s) and r["thresholds"] == ref.thresholds(s)
    assert abs(r["AP"] - ref.average_precision(y, s)) <= AP_TOL


def test_a_small_call_after_a_large_one_and_the_same_call_twice(lm, T):
    rng = np.random.default_rng(9)
    big_s, big_y = rng.integers(0, 50, 5 * T + 11), rng.integers(0, 2, 5 * T + 11)
    first = check_ranked(lm, big_s, big_y, ks=(20, 50, 100))
    check_ranked(lm, [3.0, 1.0, 2.0, 2.0, 0.5], [1, 0, 1, 0, 0], ks=(1, 2, 3, 4))   # stale workspace would show here
    again = lm.ranked(dev(big_s, torch.float32), dev(big_y), ks=(20, 50, 100))
    assert again == first                                      # every float bit for bit
    assert np.float64(again["AP"]).tobytes() == np.float64(first["AP"]).tobytes()


def test_errors_on_device_data(lm):
    s, y = dev([0.3, 0.1, 0.7, 0.2], torch.float32), dev([1, 0, 1, 0])
    with pytest.raises(ValueError, match="NaN"):
        lm.ranked(dev([0.3, float("nan"), 0.7, 0.2], torch.float32), y)
    with pytest.raises(ValueError, match="both classes"):
        lm.ranked(s, dev([1, 1, 1, 1]))
    with pytest.raises(ValueError, match="positive"):
        lm.ranked(s, dev([0, 0, 0, 0]))
    with pytest.raises(ValueError, match="0 or 1"):
        lm.ranked(s, dev([1, 0, 2, 0]))
    with pytest.raises(ValueError, match="0 or 1"):
        lm.ranked(s, dev([1.0, 0.0, 0.5, 0.0]))
    with pytest.raises(ValueError, match="one label per score"):
        lm.ranked(s, dev([1, 0, 1]))
    with pytest.raises(ValueError, match="NaN"):
        lm.hits(s, dev([float("nan")], torch.float32))
    assert lm.ranked(s, y)["AUC"] == 1.0                       # the handle is still good


def test_sixteen_million_scores_in_closed_form(lm):
    """n = 2^24 + 3 in three tie groups (score 3, 2, 1) of known class counts: AUC, AP and Hits follow from the counts, so
    no 16 M-element host sort is needed.  A count held in fp32 cannot represent the odd totals beyond 2^24."""
    n = (1 << 24) + 3
    a_pos, a_neg, b_pos, b_neg, c_pos = 1_000_001, 4_000_000, 2_000_000, 3_000_001, 3_000_000
    c_neg = n - (a_pos + a_neg + b_pos + b_neg + c_pos)
    P, Nn = a_pos + b_pos + c_pos, a_neg + b_neg + c_neg
    # laid out lowest group first, the classes of a group apart
    parts = [(1.0, 0, c_neg), (3.0, 1, a_pos), (2.0, 0, b_neg), (1.0, 1, c_pos), (3.0, 0, a_neg), (2.0, 1, b_pos)]
    s = torch.cat([torch.full((k,), v, dtype=torch.float32, device="cuda:0") for v, _, k in parts])
    y = torch.cat([torch.full((k,), lab, dtype=torch.uint8, device="cuda:0") for _, lab, k in parts])
    ks = (1, a_neg, a_neg + 1, a_neg + b_neg, a_neg + b_neg + 1, Nn, Nn + 1)
    r = lm.ranked(s, y, ks=ks)
    num = a_neg * a_pos + b_neg * (2 * a_pos + b_pos) + c_neg * (2 * (a_pos + b_pos) + c_pos)
    ap = (a_pos / P) * (a_pos / (a_pos + a_neg)) + (b_pos / P) * ((a_pos + b_pos) / (a_pos + a_neg + b_pos + b_neg)) \
        + (c_pos / P) * (P / n)
    print(f"AUC={r['AUC']!r} closed={num / (2 * P * Nn)!r} AP={r['AP']!r} closed={ap!r}")
    assert (r["num_pos"], r["num_neg"], r["thresholds"]) == (P, Nn, 3)
    assert r["AUC"] == num / (2 * P * Nn)
    assert abs(r["AP"] - ap) <= n * 2.0 ** -53
    above = {1: 0, a_neg: 0, a_neg + 1: a_pos, a_neg + b_neg: a_pos, a_neg + b_neg + 1: a_pos + b_pos, Nn: a_pos + b_pos}
    assert r["hits"] == {**{k: c / P for k, c in above.items()}, Nn + 1: 1.0}


# ---- MRR ----------------------------------------------------------------------------------------------------------------
def check_mrr(lm, pos, neg, flat=False):
    P = pos.size
    r = lm.mrr(dev(pos), dev(neg.reshape(-1) if flat else neg))
    want, rank = ref.mrr_list(pos, neg)
    got = r["mrr_list"].cpu().numpy()
    assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
    assert abs(r["MRR"] - float(np.mean(want.astype(np.float64)))) <= P * 2.0 ** -53
    for j in (1, 3, 10):
        assert r[f"hits@{j}"] == int(np.sum(rank <= j)) / P
    return r


@pytest.mark.parametrize("M", [1, 3, 63, 64, 65, 255, 256, 257, 1000, 1025])
def test_mrr_shapes(lm, M):
    """Row bases are 4-byte aligned only whenever M % 4 != 0; integer scores tie the positive often."""
    for P in (1, 2, 63, 65, 1000):
        rng = np.random.default_rng(1000 * M + P)
        span = max(2, min(M, 40))
        pos = rng.integers(0, span, P).astype(np.float32)
        neg = rng.integers(0, span, (P, M)).astype(np.float32)
        check_mrr(lm, pos, neg, flat=bool(P % 2))
        check_mrr(lm, rng.standard_normal(P).astype(np.float32), rng.standard_normal((P, M)).astype(np.float32))


def test_mrr_rows_that_tie_the_positive(lm):
    pos = np.array([0.5, 0.5, 0.5, 0.5], dtype=np.float32)
    neg = np.array([[0.1, 0.2, 0.3], [0.5, 0.2, 0.3], [0.9, 0.5, 0.5], [0.9, 0.9, 0.9]], dtype=np.float32)
    r = check_mrr(lm, pos, neg)
    assert r["mrr_list"].cpu().tolist() == [1.0, float(np.float32(1) / np.float32(1.5)),
                                            float(np.float32(1) / np.float32(3)), 0.25]
    assert (r["hits@1"], r["hits@3"], r["hits@10"]) == (0.25, 0.75, 1.0)


def test_mrr_unaligned_base_and_repeat(lm):
    rng = np.random.default_rng(4)
    P, M = 130, 37
    pos = rng.integers(0, 20, P).astype(np.float32)
    neg = rng.integers(0, 20, (P, M)).astype(np.float32)
    buf = torch.zeros(P * M + 3, dtype=torch.float32, device="cuda:0")
    buf[3:] = dev(neg.reshape(-1))
    a = lm.mrr(dev(pos), buf[3:])                              # the whole matrix starts 12 bytes past a boundary
    b = check_mrr(lm, pos, neg)
    c = lm.mrr(dev(pos), buf[3:].view(P, M))
    for other in (b, c):
        assert a["MRR"] == other["MRR"] and torch.equal(a["mrr_list"], other["mrr_list"])


def test_mrr_errors(lm):
    pos = dev([0.5, 0.2, 0.1], torch.float32)
    with pytest.raises(ValueError, match="per positive"):
        lm.mrr(pos, torch.zeros(7, device="cuda:0"))
    with pytest.raises(ValueError, match="NaN"):
        lm.mrr(pos, dev([0.1, float("nan"), 0.3], torch.float32))
    with pytest.raises(ValueError, match="NaN"):
        lm.mrr(dev([0.5, float("nan"), 0.1], torch.float32), torch.zeros(6, device="cuda:0"))
    with pytest.raises(ValueError, match="positive"):
        lm.mrr(torch.zeros(0, device="cuda:0"), torch.zeros(6, device="cuda:0"))


def test_reference_twins_on_device_tensors(lm):
    from s3grl_amd import metrics

    rng = np.random.default_rng(11)
    pv, nv = rng.integers(0, 30, 150).astype(np.float32), rng.integers(0, 25, 450).astype(np.float32)
    pt, nt = rng.integers(0, 30, 90).astype(np.float32), rng.integers(0, 25, 270).astype(np.float32)
    yv, yt = np.r_[np.ones(150), np.zeros(450)], np.r_[np.ones(90), np.zeros(270)]
    sv, st = np.r_[pv, nv], np.r_[pt, nt]
    r = metrics.evaluate_auc(dev(sv), dev(yv), dev(st), dev(yt))
    assert set(r) == {"AUC", "AP"}
    assert r["AUC"] == (ref.roc_auc_exact(yv, sv), ref.roc_auc_exact(yt, st))
    assert abs(r["AP"][0] - ref.average_precision(yv, sv)) <= AP_TOL
    assert abs(r["AP"][1] - ref.average_precision(yt, st)) <= AP_TOL
    h = metrics.evaluate_hits(dev(pv), dev(nv), dev(pt), dev(nt), evaluator=object())
    assert h == {f"Hits@{k}": (ref.hits_at(pv, nv, k), ref.hits_at(pt, nt, k)) for k in (20, 50, 100)}
    q = metrics.evaluate_mrr(dev(pv), dev(nv), dev(pt), dev(nt))
    assert abs(q["MRR"][0] - ref.mrr(pv, nv.reshape(150, 3))["MRR"]) <= 150 * 2.0 ** -53
    assert abs(q["MRR"][1] - ref.mrr(pt, nt.reshape(90, 3))["MRR"]) <= 90 * 2.0 ** -53
    assert metrics.evaluate_ogb_rocauc(dev(pv), dev(nv), dev(pt), dev(nt)) == {"rocauc": r["AUC"]}
