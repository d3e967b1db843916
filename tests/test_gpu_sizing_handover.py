"""-m gpu: the sizing pass from cached balls (`count_balls_kernel`, csrc/s3grl_balls.hip) and its hand-over
to the link kernels and the gather, at the shapes where its word ownership, its scans and its LDS window
change path.

The yardstick is the other sizing pass: the same plans with the ball cache on and with S3GRL_NO_BALL_CACHE=1
(a BFS per link, `count_kernel`) must agree bit for bit in everything a plan hands out — node lists and
distances (`export_subgraphs`), `row_ptr`, `row_nodes`, the statistics and the rows of `run()`.

`count_balls_kernel` deals the W = ceil(N / 32) bitmap words of a level round-robin to T threads, CW = ceil(W / T)
words each (the launcher takes the smallest T in 64, 128, .. with W <= 5 T), places a level's nodes in an LDS
window of 1 024 entries and copies the window to the link's stash slot; what a level has beyond the window is
stored node by node, and nothing is stored beyond the slot (4 096 entries, S3GRL_STASH_SLOT).  The shapes:

  n33      W = 2     threads without a word, a partly filled last word
  n300     W = 10    the same, more than one word per row
  n2100    W = 66    T = 64, two chunks, the second with 2 words
  n10300   W = 322   T = 128 (two waves: the table of wave totals), three chunks, the last one partial:
                     the launch shape of the headline; mean degree 3, 40 links
  star     3 000 leaves and a few pendant paths, links at the centre: one level of more than 1 024 nodes;
           with S3GRL_STASH_SLOT=16 too, where a level overruns its slot
  edge     isolated endpoints (a level that is empty at once), endpoints in one bitmap word, reversed
           duplicates in the list (folded links)

each at num_hops 1, 2 and 3, for PoS and PoS Plus.  Lists that are gathered in pieces (S3GRL_SPLIT_T,
S3GRL_SPLIT_SEG_SHIFT set small) go through the same comparison, agree with the unsplit plan within the
tolerance of tests/test_gpu_parity.py, and `plan.run` is called right after `eng.plan` returns, before any
statistic is read.

The link kernels behind the two sizing passes are not always the same: on a graph of more than 8 192 nodes a
plain plan whose operators all reach the whole subgraph (sign_k - 1 >= num_hops) runs `link_csr_kernel` when
the graph has cached balls and `link_kernel` when it has none (`csr_mode_for`, csrc/s3grl_csr.hip), and the two
sum a row's terms in different orders: n10300 at 2 hops, PoS, sign_k 3 differs in 42 elements of 4 of its 80
rows by one unit in the last place (2.4e-07), before and after the round-robin kernel.  So every shape is
compared twice: with S3GRL_NO_CSR=1 in both flavours, where the link kernels are the same and everything is
bit for bit; and as the engine runs by default, where everything but the rows is bit for bit and the rows agree
within the tolerance of tests/test_gpu_parity.py.
"""
import os

import numpy as np
import pytest

from conftest import csr_from_undirected

pytestmark = pytest.mark.gpu

HOOKS = ("S3GRL_NO_CSR", "S3GRL_NO_BALL_CACHE", "S3GRL_BALL_CACHE_BYTES", "S3GRL_STASH_SLOT", "S3GRL_SPLIT_T",
         "S3GRL_SPLIT_SEG_SHIFT")
HOPS = (1, 2, 3)
MODES = {"pos": 3, "pos_plus": 2}   # mode -> sign_k


@pytest.fixture(scope="module")
def eng():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    e = Engine("cuda:0")
    yield e
    e.close()


def random_graph(n, mean_degree, seed, n_links):
    rng = np.random.default_rng(seed)
    m = int(n * mean_degree / 2)
    e = rng.integers(0, n, size=(m, 2))
    e = e[e[:, 0] != e[:, 1]]
    # links: half of them edges (their endpoints are neighbours), half random pairs
    pos = e[rng.choice(len(e), n_links // 2, replace=False)]
    neg = rng.integers(0, n, size=(n_links, 2))
    neg = neg[neg[:, 0] != neg[:, 1]][:n_links - len(pos)]
    return n, e, np.concatenate([pos, neg])


def star_graph():
    leaves, paths, plen = 3000, 4, 3
    edges = [(0, 1 + i) for i in range(leaves)]
    n = 1 + leaves
    tips = []
    for _ in range(paths):          # pendant paths off the centre
        prev = 0
        for _ in range(plen):
            edges.append((prev, n))
            prev = n
            n += 1
        tips.append(prev)
    links = [(0, 1), (0, tips[0]), (tips[1], 0), (5, 7), (tips[2], tips[3]), (2999, tips[0]), (0, tips[0] - 1)]
    return n, np.array(edges), np.array(links)


def edge_graph():
    n = 70   # W = 3; 66 .. 69 have no edge
    rng = np.random.default_rng(5)
    e = rng.integers(0, 66, size=(90, 2))
    e = e[e[:, 0] != e[:, 1]]
    links = [(68, 69), (67, 3), (3, 67), (0, 1), (1, 0), (e[0, 0], e[0, 1]), (e[0, 1], e[0, 0]), (2, 40), (40, 2),
             (64, 65), (31, 32), (66, 67)]
    return n, e, np.array(links)


SHAPES = {
    "n33": lambda: random_graph(33, 3, 1, 12),
    "n300": lambda: random_graph(300, 3, 2, 20),
    "n2100": lambda: random_graph(2100, 3, 3, 24),
    "n10300": lambda: random_graph(10300, 3, 4, 40),
    "star": star_graph,
    "edge": edge_graph,
}

_cache = {}


def outputs(eng, shape, env):
    """Everything the plans of one shape hand out, per (num_hops, mode), with the hooks of `env` set while the
    graph and the plans are created; computed once per (shape, env)."""
    key = (shape, tuple(sorted(env.items())))
    if key in _cache:
        return _cache[key]
    n, edges, links = SHAPES[shape]()
    A = csr_from_undirected(n, edges)
    A.data[:] = 1
    X = np.random.default_rng(11).standard_normal((n, 9))
    saved = {k: os.environ.pop(k, None) for k in HOOKS}
    os.environ.update(env)
    try:
        f = eng.features(X)
        L = eng.links(links.T)
        G = eng.graph(A)
        res = {}
        for hops in HOPS:
            for mode, K in MODES.items():
                p = eng.plan(G, L, mode=mode, num_hops=hops, sign_k=K, full_stats=(hops == 2))
                rows = p.run(f).clone()    # right after plan(): no statistic has been read
                st = dict(p.stats)
                st.pop("workspace_bytes")
                res[(hops, mode)] = ([t.clone() for t in p.export_subgraphs()], p.row_ptr().clone(),
                                     p.row_nodes().clone(), st, rows)
                p.close()
        G.close()
        f.close()
    finally:
        for k in HOOKS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]
    _cache[key] = res
    return res


def rows_diff(ra, rb):
    """what differs between two row tensors, for the assertion message"""
    import torch

    if ra.shape != rb.shape:
        return f"shapes {tuple(ra.shape)} / {tuple(rb.shape)}"
    bad = (ra != rb) & ~(torch.isnan(ra) & torch.isnan(rb))
    rows = torch.nonzero(bad.flatten(1).any(1)).flatten().tolist()
    return (f"{int(bad.sum())} elements in {len(rows)} of {ra.shape[0]} rows (first rows {rows[:6]}), "
            f"max |a - b| {float((ra - rb).abs().nan_to_num().max()):.3e}, NaNs {int(torch.isnan(ra).sum())} / "
            f"{int(torch.isnan(rb).sum())}")


def assert_same_plan(a, b, what):
    import torch

    (ea, pa, na, sa, ra), (eb, pb, nb, sb, rb) = a, b
    assert len(ea) == len(eb) and all(torch.equal(x, y) for x, y in zip(ea, eb)), what + ": subgraphs"
    assert torch.equal(pa, pb), what + ": row_ptr"
    assert torch.equal(na, nb), what + ": row_nodes"
    assert sa == sb, what + ": stats"
    assert (ra is None and rb is None) or torch.equal(ra, rb), what + ": rows: " + rows_diff(ra, rb)


def assert_same_rows(a, b, what):
    import torch

    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), what + ": row_ptr / row_nodes"
    assert torch.equal(a[4], b[4]), what + ": rows: " + rows_diff(a[4], b[4])


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sizing_from_balls_equals_the_bfs(eng, shape, hops, mode):
    from test_gpu_parity import TOL, rel_err

    what = f"{shape} {hops} hops {mode}"
    same_kernels = {"S3GRL_NO_CSR": "1"}
    balls = outputs(eng, shape, same_kernels)[(hops, mode)]
    bfs = outputs(eng, shape, dict(same_kernels, S3GRL_NO_BALL_CACHE="1"))[(hops, mode)]
    assert int(balls[1][-1]) > 0
    assert_same_plan(balls, bfs, what + ", link_kernel in both")
    by_default = outputs(eng, shape, {})[(hops, mode)]
    assert_same_plan(by_default[:4] + (None,), bfs[:4] + (None,), what + ", default")
    assert by_default[4].shape == bfs[4].shape
    assert rel_err(by_default[4].cpu().numpy(), bfs[4].cpu().numpy()) <= TOL, what + ", default: rows"


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("hops", HOPS)
@pytest.mark.parametrize("shape", ["star", "n300"])
def test_level_that_overruns_its_slot(eng, shape, hops, mode):
    """A slot of 16 entries: the lists are cut, the link kernels walk the graph again where the list does not
    fit, and the plan hands out what it hands out with the whole list."""
    cut = outputs(eng, shape, {"S3GRL_STASH_SLOT": "16"})[(hops, mode)]
    cut_bfs = outputs(eng, shape, {"S3GRL_STASH_SLOT": "16", "S3GRL_NO_BALL_CACHE": "1"})[(hops, mode)]
    assert_same_plan(cut, cut_bfs, f"{shape} {hops} hops {mode}, slot 16")
    assert_same_rows(cut, outputs(eng, shape, {})[(hops, mode)], f"{shape} {hops} hops {mode}, slot 16 vs 4096")


SPLIT = {"S3GRL_SPLIT_T": "32", "S3GRL_SPLIT_SEG_SHIFT": "4"}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("hops", (2, 3))
def test_lists_gathered_in_pieces(eng, hops, mode):
    """Lists of more than 32 entries in pieces of 16: the same bits from both sizing passes and with a slot the
    lists overrun, and the rows of the unsplit plan within the parity tolerance (the pieces change the order of
    the float sums)."""
    from test_gpu_parity import TOL, rel_err

    shape = "n2100"
    split = outputs(eng, shape, SPLIT)[(hops, mode)]
    assert_same_plan(split, outputs(eng, shape, dict(SPLIT, S3GRL_NO_BALL_CACHE="1"))[(hops, mode)],
                     f"split, {hops} hops {mode}: balls vs bfs")
    assert_same_rows(split, outputs(eng, shape, dict(SPLIT, S3GRL_STASH_SLOT="16"))[(hops, mode)],
                     f"split, {hops} hops {mode}: slot 16")
    whole = outputs(eng, shape, {"S3GRL_SPLIT_T": "0"})[(hops, mode)]
    import torch

    assert torch.equal(split[1], whole[1]) and torch.equal(split[2], whole[2])
    assert int(torch.diff(split[0][0]).max()) > 32    # (some list is in pieces)
    err = rel_err(split[4].cpu().numpy(), whole[4].cpu().numpy())
    print(f"[sizing] split vs unsplit, {hops} hops {mode}: rel err {err:.2e}")
    assert err <= TOL
