"""Host checks of the prefix-schedule tests' inputs (test_gpu_gather_prefix.py): a numpy BFS over the broom
graphs of prefix_graphs.py shows that every intended prefix length, and every "list ends inside / one to three
rows after phase A" case, is really produced; and the single-rounded fp32 multiply-add the GPU test sums with
is checked against exact rational arithmetic."""
from fractions import Fraction

import numpy as np

import prefix_graphs as pg
from prefix_fma import fma32


def _sizes(reversed_links=False):
    n, edges, links = pg.brooms(reversed_links=reversed_links)
    return [[len(h) for h in pg.hop_lists(n, edges, l)] for l in links]


def test_hop_sizes_are_the_tables():
    sizes = _sizes()
    assert len(sizes) == len(pg.SHAPES)
    for (n1, n2, n3), s in zip(pg.SHAPES, sizes):
        assert s == [2, n1, n2, n3]
    rev = _sizes(reversed_links=True)
    assert rev[0::2] == sizes and rev[1::2] == sizes


def test_every_prefix_length_with_a_last_hop_beyond():
    sizes = _sizes()
    k3 = {2 + s[1] + s[2] for s in sizes if s[3] >= 2 * pg.U}   # a phase B of at least one whole group
    assert set(pg.PREFIX_LENGTHS) <= k3
    k2 = {2 + s[1] for s in sizes if s[2] >= 2 * pg.U}
    assert set(pg.SIGN_K2_PREFIX_LENGTHS) <= k2
    # 1, 2, 3: the part of a prefix that falls into the second piece of a list gathered in pieces of SEG rows
    piece = {2 + s[1] + s[2] - pg.SEG for s in sizes if sum(s) > 48}
    assert set(pg.PIECE_PREFIX_LENGTHS) <= piece


def test_lists_that_end_inside_and_just_after_phase_a():
    sizes = _sizes()
    for i in pg.ENDS_INSIDE_A:
        s = sizes[i]
        rows, inside = pg.phase_a_rows(2 + s[1] + s[2], sum(s))
        assert inside and rows == sum(s) and s[3] >= 1
    for i, after in pg.ENDS_AFTER_A.items():
        s = sizes[i]
        rows, inside = pg.phase_a_rows(2 + s[1] + s[2], sum(s))
        assert not inside and sum(s) - rows == after
    assert sorted(pg.ENDS_AFTER_A.values()) == [1, 2, 3]
    # ... and a window's edge among them
    assert any(2 + sizes[i][1] + sizes[i][2] > pg.W for i in pg.ENDS_INSIDE_A)
    assert any(2 + sizes[i][1] + sizes[i][2] == pg.W for i in pg.ENDS_AFTER_A)


def _fma_exact(a, b, c):
    """round-to-nearest-even fp32 of the exact a * b + c, by rational arithmetic"""
    x = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    if x == 0:
        return np.float32(0.0)
    f = np.float32(float(x))   # float(Fraction) rounds once to 53 bits: only a first guess
    cands = {f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))}
    best = min(cands, key=lambda t: (abs(Fraction(float(t)) - x), int(np.float32(t).view(np.uint32)) & 1))
    return np.float32(best)


def test_fma32_is_single_rounded():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(np.float32)
    # a sum that lands ON a tie of the fp32 rounding once it is rounded to 53 bits, though the exact one lies
    # below it: c = 1 + 2^-23, a * b = 2^-24 (1 - 2^-30); and signed zeros
    a = np.concatenate([a, np.float32([1 + 2.0 ** -15, 0.0, -1.5])])
    b = np.concatenate([b, np.float32([2.0 ** -24 * (1 - 2.0 ** -15), 3.0, 2.0])])
    c = np.concatenate([c, np.float32([1 + 2.0 ** -23, -0.0, 3.0])])
    naive = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    got = fma32(a, b, c)
    assert got.dtype == np.float32
    ref = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    # neither the fp32 two-step form nor a plain fp64 sum is that: the check is not vacuous
    assert not np.array_equal((a * b + c).astype(np.float32).view(np.uint32), ref.view(np.uint32))
    assert naive[4000] != ref[4000]
