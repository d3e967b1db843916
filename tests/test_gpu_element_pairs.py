"""-m gpu: the paired fetch of the packed gather's split phase B (el_phase_b: two element rows per 16-byte
wave-load, lanes 0-31 the first row and lanes 32-63 the second, two v_permlane32_swap) and the element-row layout
it reads (el_fill_kernel: even starts, even sizes, a padding entry, the first 64 entries of a row interleaved
for the two half-waves) — which the one-launch kernels read too, one row per load.

Broom graphs (prefix_graphs.py) put the phase-B part of a list on every length that matters to the pairing:
4 .. 7 rows (one group, with and without an odd last row), 63 .. 66 and 127 .. 129 (the edges of a window of 64
rows, a single pair after it).  The operand gives node v in tile t a chosen number of entries, cycling through
0, 64, 1, 2, 65, 3, 31, 32, 128, 33, 63, 129, 127 — an odd cycle, so neighbours in a list pair up in both orders:
(empty, full), (odd, even), (more than 64, short) and their mirrors.  The heavy operand holds the cycle in every
node (about 52 entries per row-tile: the two-launch plan, kernels <K,1,2> + <K,1,3>), the light one in every
third node (below 24: the one-launch kernel <K,1,1>).

`auto` (element rows) and `packed_only` (chunks) must agree BIT FOR BIT: a row's columns are distinct, so
where an entry sits in its row changes no column's summation order.  Both are held to the dense operand within
1e-6 of the row norm, the bound of test_gpu_gather_prefix.py.  plan.gather_traffic tells which kernels ran.

Mutations of el_phase_b this file caught when it was written (each built once, run once, not kept): the swap of
the slot dwords left out; the second row of a pair fetched from the first row's start (DESIGN.md Part II has
the counts)."""
import functools

import numpy as np
import pytest

import prefix_graphs as pg
from conftest import csr_from_undirected

pytestmark = pytest.mark.gpu

HOPS = 3
ATOL = 1e-10
COUNTS = [0, 64, 1, 2, 65, 3, 31, 32, 128, 33, 63, 129, 127]   # entries per row-tile, in node order
LENGTHS = [4, 5, 6, 7, 63, 64, 65, 66, 127, 128, 129]          # rows of a list beyond phase A
SPLIT_MIN = 24      # kSplitMinEntries of s3grl_packed.hip: average entries per row-tile of the two-launch plan
SPLIT_T = 48        # the hooks of the `pieces` cases (as test_gpu_element_split.py sets them)


@pytest.fixture(scope="module")
def eng():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    e = Engine("cuda:0")
    yield e
    e.close()


def _shapes(K):
    """Brooms whose list has L rows beyond phase A at sign_k = K, for every L of LENGTHS.  Phase A ends with the
    group of four rows that holds the prefix's last row: sign_k 3: prefix 2 + 1 + 1 = 4, then the L nodes of
    hop 3; sign_k 2: prefix 2 + 1 = 3 of a list of 3 + (L + 1) rows; sign_k 1: no prefix, a list of 2 + (L - 2)."""
    if K == 3:
        return [(1, 1, L) for L in LENGTHS]
    if K == 2:
        return [(1, L + 1, 1) for L in LENGTHS]
    return [(L - 2, 1, 1) for L in LENGTHS]


@functools.lru_cache(maxsize=None)
def _scene(K):
    n, edges, links = pg.brooms(_shapes(K))
    links = np.concatenate([links, links[::2, ::-1]])     # every other link once more, reversed: folded
    A = csr_from_undirected(n, edges)
    for (n1, n2, n3), l in zip(_shapes(K), links):
        sizes = [len(h) for h in pg.hop_lists(n, edges, l)[:K + 1]]
        assert sizes == [2, n1, n2, n3][:K + 1]
        prefix = sum(sizes[:K]) if K > 1 else 0
        assert sum(sizes) - (prefix + pg.U - 1) // pg.U * pg.U in LENGTHS
    return n, A, links


@functools.lru_cache(maxsize=None)
def _operand(n, F, heavy):
    rng = np.random.default_rng(F + heavy)
    X = np.zeros((n, F), dtype=np.float32)
    tiles = (F + 511) // 512
    for v in range(n):
        for t in range(tiles):
            cols = min(512, F - 512 * t)
            if heavy:
                c = COUNTS[(v + 5 * t) % len(COUNTS)]
            else:
                c = COUNTS[(v // 3 + 5 * t) % len(COUNTS)] if v % 3 == 0 else (v + t) % 4
            c = min(c, cols)
            val = rng.standard_normal(c).astype(np.float32)
            val[val == 0] = 1.0
            X[v, 512 * t + rng.choice(cols, size=c, replace=False)] = val
    per_tile = (X != 0).sum() / (n * tiles)
    # (the library counts a padding entry per odd row-tile on top: below 0.5)
    assert per_tile >= SPLIT_MIN if heavy else per_tile + 0.5 < SPLIT_MIN
    return X


def rel_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=-1, keepdims=True))
    return float(np.max(np.clip(np.abs(got - ref) - ATOL, 0, None) / np.maximum(scale, 1e-30)))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(eng, monkeypatch, K, F, heavy, mode, split):
    n, A, links = _scene(K)
    X = _operand(n, F, heavy)
    if split:
        monkeypatch.setenv("S3GRL_SPLIT_T", str(SPLIT_T))
        monkeypatch.setenv("S3GRL_SPLIT_SEG_SHIFT", "4")
    G = eng.graph(A)
    plan = eng.plan(G, eng.links(links.T.copy()), mode=mode, num_hops=HOPS, sign_k=K)
    try:
        assert plan.folded_links == (len(LENGTHS) + 1) // 2
        if split:
            assert plan.stats["max_nodes"] > SPLIT_T
        got, traffic = {}, {}
        for fmode in ("auto", "packed_only", "dense"):
            f = eng.features(X, fmode)
            assert f.is_packed == (fmode != "dense") and not f.is_sparse
            got[fmode] = plan.run(f).cpu().numpy()
            if fmode != "dense":
                traffic[fmode] = plan.gather_traffic(f)
            f.close()
        # which kernels ran: only the two-launch element plan fetches 8 header bytes (the element range) instead
        # of 32 for the rows of its phase-B launch; the element rows are fewer bytes than the chunks
        t = traffic["auto"]
        assert (t["headers"] < 8 * t["ids"]) == heavy, t
        assert not traffic["packed_only"]["headers"] < 8 * traffic["packed_only"]["ids"]
        assert t["features"] < traffic["packed_only"]["features"], (t, traffic["packed_only"])
        bad = np.argwhere(_bits(got["auto"]) != _bits(got["packed_only"]))
        print("differing outputs: %d of %d" % (len(bad), got["auto"].size))
        assert not len(bad), (len(bad), bad[:4].tolist(), got["auto"][tuple(bad[0])], got["packed_only"][tuple(bad[0])])
        for fmode in ("auto", "packed_only"):
            err = rel_err(got[fmode], got["dense"])
            assert err < 1e-6, (fmode, err)
    finally:
        plan.close()
        G.close()


@pytest.mark.parametrize("heavy", [True, False], ids=["two_launches", "one_launch"])
@pytest.mark.parametrize("F", [500, 512, 513, 1030])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_pairs_bits(eng, monkeypatch, K, F, heavy):
    """One, two and three tiles, a last tile of one and of six columns."""
    _check(eng, monkeypatch, K, F, heavy, "pos", False)


@pytest.mark.parametrize("heavy", [True, False], ids=["two_launches", "one_launch"])
@pytest.mark.parametrize("K", [1, 2, 3])
def test_pairs_pieces(eng, monkeypatch, K, heavy):
    """The lists of more than 48 rows gathered in pieces of 16: every piece its own phase B."""
    _check(eng, monkeypatch, K, 1030, heavy, "pos", True)


@pytest.mark.parametrize("K", [2, 3])
def test_pairs_pos_plus(eng, monkeypatch, K):
    """A second row pair per link (the common neighbour), whose list reaches one hop further."""
    _check(eng, monkeypatch, K, 513, True, "pos_plus", False)
