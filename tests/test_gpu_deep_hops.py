"""-m gpu: subgraphs deeper than three hops (num_hops 4 .. 30) against the fp64 restatements.

Every input is built from seeded numpy; every reference is computed at test time by the plain-C
restatement (oracle.c_oracle) or the Python oracle.  The generated graphs (tests/deep_graphs.py):

  grid   a 12 x 25 grid with a few random chords: every hop adds a level of its own, so the per-operator
         list limits job_lim[0 .. K-1] of a job are all distinct and the list prefixes are long
  rand   the rand300 fixture graph: small diameter, the lists saturate at hops >= 4 and several trailing
         limits coincide (nb >= 2 inside the element kernels)
  path   80 nodes in a line, links near the middle: num_hops = 30 fills all 31 levels
  ring   40 nodes in a cycle: with one endpoint masked, distances go the long way round (beyond the hop
         count; beyond 2 * hops they cannot go on a ring, which lies inside the subgraph only when n <= 2 * hops + 2)
  fan    dst joined to every node of a 150-node path, src to its first node: with dst masked, src reaches the
         path's far end in 150 steps at any depth (beyond 2 * hops, and beyond DE+'s clamp at 100)

The gather matrix runs sign_k 1..8 at hops max(1, K - 1) (every job's trailing operators reach its whole
list: the MINNB = 2 packed kernel), K (the element kernels) and 8, on every feature operand.  Which kernel a
case reaches is decided by the plan and the operand alone; `Plan.gather_traffic` (gather_traffic_kernel in
csrc/s3grl_packed.hip, the same phase arithmetic as the kernels) is the witness, see `_witness`.
"""
import numpy as np
import pytest

from conftest import csr_from_undirected
from deep_graphs import GRAPHS, grid_graph, path_graph
from oracle import c_oracle

pytestmark = pytest.mark.gpu

TOL = 1e-5          # the parity bar of test_gpu_parity.py
ATOL = 1e-10
TERMS_ULPS = 0.2    # the fuzz sweep's allowance for signed features: 2e-6 of the sum of the |terms|


# ---- helpers --------------------------------------------------------------------------------------------

def rel_err(got, ref, terms=None):
    """Row-norm relative error (test_gpu_fuzz.rel_err): `terms`, the same rows on |X|, widens the scale by a
    few ulps of the sum of the absolute terms where signed features cancel."""
    ref = np.asarray(ref, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    if not ref.size:
        return 0.0
    scale = np.maximum(np.abs(ref), np.abs(ref).max(axis=-1, keepdims=True))
    if terms is not None:
        scale = np.maximum(scale, TERMS_ULPS * np.abs(terms))
    return float(np.max(np.clip(np.abs(got - ref) - ATOL, 0, None) / np.maximum(scale, 1e-30)))


def assert_parity(got, A, links, hops, X, K, plus, ref):
    """got against the fp64 rows `ref`; on a miss, judged once more against the sum of the |terms|."""
    got = got.cpu().numpy()
    err = rel_err(got, ref)
    if err >= TOL:      # cancellation of signed features?
        terms = c_oracle.pos_rows(links.T, hops, A, np.abs(X), K, plus=plus)[0]
        err = rel_err(got, ref, terms)
    assert err < TOL, (hops, K, plus, X.shape, err)


@pytest.fixture(scope="module")
def eng():
    import torch
    from s3grl_amd.engine import Engine

    assert torch.cuda.is_available()
    e = Engine("cuda:0")
    yield e
    e.close()


def operands(n, seed):
    """Feature matrices of the gather matrix (signed): 'narrow' F = 100 and 'one' F = 200 (dense operand
    only), 'lo' and 'hi' F = 515 (two packed tiles of 512 columns; every operand).  Both sparse ones hold a
    fully dense row (515 entries: more than 64 in a tile), an empty row and a row with an entry in every
    third column; 'lo' has fewer than kSplitMinEntries = 24 element entries per row-tile on average (the
    one-launch element kernel <K,1,1>), 'hi' more (<K,1,2> + the phase-B launch <K,1,3>)."""
    rng = np.random.default_rng(seed)
    out = {"narrow": rng.standard_normal((n, 100)), "one": rng.standard_normal((n, 200))}
    for name, density in (("lo", 0.04), ("hi", 0.15)):
        X = rng.standard_normal((n, 515)) * (rng.random((n, 515)) < density)
        X[7] = rng.standard_normal(515)
        X[11] = 0
        X[13, ::3] = rng.random(172) + 0.5
        out[name] = X
    out = {k: v.astype(np.float32) for k, v in out.items()}
    tiles = 2
    assert np.count_nonzero(out["lo"]) < 24 * n * tiles <= np.count_nonzero(out["hi"])
    return out


class Setup:
    """One graph with its features prepared once for every operand mode."""

    def __init__(self, eng, name):
        self.n, edges, self.links = GRAPHS[name]()
        self.A = csr_from_undirected(self.n, edges)
        self.G = eng.graph(self.A)
        self.L = eng.links(self.links.T.copy())
        self.X = operands(self.n, 17)
        self.f = {("narrow", "dense"): eng.features(self.X["narrow"], "dense"),
                  ("one", "dense"): eng.features(self.X["one"], "dense")}
        for x in ("lo", "hi"):
            for m in ("dense", "packed", "packed_only", "sparse"):
                self.f[(x, m)] = eng.features(self.X[x], m)
                assert self.f[(x, m)].is_packed == m.startswith("packed")
                assert self.f[(x, m)].is_sparse == (m == "sparse")

    def close(self):
        for f in self.f.values():
            f.close()
        self.G.close()


@pytest.fixture(scope="module")
def setups(eng):
    s = {}
    yield lambda name: s[name] if name in s else s.setdefault(name, Setup(eng, name))
    for v in s.values():
        v.close()


def element_mode(K, hops):
    """element_mode() of csrc/s3grl_packed.hip for an operand with element rows: 0 when every job's last
    two operators reach its whole list (sign_k - 1 >= depth), else on (1 or 2 by the entries per tile)."""
    return not (K >= 2 and K - 1 >= hops)


def _witness(plan, S, K, hops, strict):
    """The kernel each packed operand reached, read off Plan.gather_traffic (gather_traffic_kernel):

    * element rows off (sign_k - 1 >= hops): 'packed' and 'packed_only' request the same bytes, every count.
    * element rows on, one launch ('lo', <K,1,1>): every job whose phase B (the last operator beyond the
      prefix the others reach) is non-empty fetches those rows as 8 bytes per element entry instead of 16 per
      non-zero chunk, so `features` differs; nothing else is written or reread: `output`, `x_rows` and
      `headers` are equal.
    * element rows on, phase B split off ('hi', <K,1,2> then <K,1,3>): each job with nb == 1 (one trailing
      operator reaches the whole list) and a non-empty phase B writes its fp32 partial rows in phase A and
      reads them back in phase B: `output` and `x_rows` on 'packed' both exceed 'packed_only' by the same
      4 * F * (rows of those jobs) bytes.
    `strict` (the grid: every hop adds a distinct level, so at hops >= K every job has nb == 1 and a long
    phase B) requires the difference to be there; on a saturated graph it may be zero (nb >= 2 everywhere).
    The dense operand: F = 100 is gathered by gather_narrow_kernel<K> (F <= 128), F = 200 by
    gather_kernel<K,1> (one 256-column tile), F = 515 by gather_kernel<K,2> in two 512-column tiles."""
    t = {k: plan.gather_traffic(S.f[k]) for k in S.f if k[1] != "sparse"}
    assert t[("hi", "dense")]["waves"] == 2 * t[("one", "dense")]["waves"] == 2 * t[("narrow", "dense")]["waves"]
    lo, lo0 = t[("lo", "packed")], t[("lo", "packed_only")]
    hi, hi0 = t[("hi", "packed")], t[("hi", "packed_only")]
    if not element_mode(K, hops):
        assert lo == lo0 and hi == hi0
        return
    assert lo["output"] == lo0["output"] and lo["x_rows"] == lo0["x_rows"] and lo["headers"] == lo0["headers"]
    d = hi["output"] - hi0["output"]
    assert d == hi["x_rows"] - hi0["x_rows"] and d >= 0 and d % (4 * 515) == 0
    if strict:
        assert lo["features"] != lo0["features"]
        assert d > 0


def _check_plan(plan, S, K, hops, plus, strict=True):
    import torch

    ref = {x: c_oracle.pos_rows(S.links.T, hops, S.A, S.X[x], K, plus=plus) for x in S.X}
    _, ptr, nodes, _ = ref["lo"]
    np.testing.assert_array_equal(plan.row_ptr().cpu().numpy(), ptr)
    np.testing.assert_array_equal(plan.row_nodes().cpu().numpy(), nodes)
    out = {}
    for (x, m), f in S.f.items():
        out[(x, m)] = plan.run(f)
        assert_parity(out[(x, m)], S.A, S.links, hops, S.X[x], K, plus, ref[x][0])
    for x in ("lo", "hi"):
        assert torch.equal(out[(x, "packed")], out[(x, "packed_only")]), x     # element rows: the same bits
        assert rel_err(out[(x, "packed")].cpu().numpy(), out[(x, "dense")].cpu().numpy()) < 1e-6
    _witness(plan, S, K, hops, strict)


MATRIX = [(K, h) for K in range(1, 9) for h in sorted({max(1, K - 1), K, 8})]


@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
@pytest.mark.parametrize("K,hops", MATRIX)
@pytest.mark.parametrize("name", ["grid", "rand"])
def test_gather_matrix(eng, setups, name, K, hops, mode):
    """sign_k 1..8 at hops max(1, K - 1) (the MINNB = 2 packed kernel), K (element kernels) and 8, every
    operand of one plan against the fp64 rows; 'packed' against 'packed_only' bit for bit and against
    'dense' to 1e-6; the kernel each reached by the traffic witness (_witness)."""
    S = setups(name)
    plan = eng.plan(S.G, S.L, mode=mode, num_hops=hops, sign_k=K)
    try:
        _check_plan(plan, S, K, hops, mode == "pos_plus", strict=name == "grid" and hops >= K)
        assert plan.stats["folded_links"] >= 2       # the reversed duplicates
    finally:
        plan.close()


@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
@pytest.mark.parametrize("K,hops", [(4, 4), (4, 8), (6, 6), (6, 8), (8, 8)])
@pytest.mark.parametrize("name", ["grid", "rand"])
def test_gather_in_pieces(eng, setups, monkeypatch, name, K, hops, mode):
    """The same checks with the long lists gathered in pieces of 32 (partial rows combined afterwards):
    phase B of the element plans then reads and writes the pieces' partial rows."""
    monkeypatch.setenv("S3GRL_SPLIT_T", "64")           # read when a plan is made: graph and operands are shared
    monkeypatch.setenv("S3GRL_SPLIT_SEG_SHIFT", "5")
    S = setups(name)
    plan = eng.plan(S.G, S.L, mode=mode, num_hops=hops, sign_k=K)
    try:
        _check_plan(plan, S, K, hops, mode == "pos_plus", strict=name == "grid")
        assert plan.stats["max_nodes"] > 64
    finally:
        plan.close()


# ---- structure at depth ---------------------------------------------------------------------------------

def small_x(n, seed=3):
    return np.abs(np.random.default_rng(seed).standard_normal((n, 9))).astype(np.float32)


def plan_classes(eng, G, L, **kw):
    """Links per class of a plan, as the plan prints them under S3GRL_DEBUG (test_gpu_csr.py's witness:
    lists 32 .. 45 are the induced-CSR classes)."""
    import os
    import re
    import tempfile

    os.environ["S3GRL_DEBUG"] = "1"
    try:
        with tempfile.TemporaryFile(mode="w+b") as tmp:
            saved = os.dup(2)
            os.dup2(tmp.fileno(), 2)
            try:
                eng.plan(G, L, **kw).close()
            finally:
                os.dup2(saved, 2)
                os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode()
    finally:
        del os.environ["S3GRL_DEBUG"]
    m = re.search(r"classes:((?: -?\d+)+)", text)
    assert m, text
    return [int(x) for x in m.group(1).split()]


def _check_structure(eng, G, A, links, hops, K, mode="pos_plus"):
    """export_subgraphs() against c_oracle.extract (node sets, hop-major order and dists exact) and the rows
    of a dense F = 9 operand against the fp64 rows (row pointers and row nodes exact).  The plan keeps full
    stats, as test_subgraph_node_sets_bit_exact does: every link (reversed duplicates too) is extracted and
    exported on its own.  The export orders hop 0 like any other hop, by ascending id."""
    plus = mode == "pos_plus"
    X = small_x(A.shape[0])
    plan = eng.plan(G, eng.links(links.T.copy()), mode=mode, num_hops=hops, sign_k=K, full_stats=True)
    try:
        f = eng.features(X, "dense")
        rows = plan.run(f)
        node_ptr, nodes, dists = (t.cpu().numpy() for t in plan.export_subgraphs())
        ref_ptr, ref_nodes, ref_dists = c_oracle.extract(links.T, hops, A)
        first = ref_ptr[:-1]
        ref_nodes[first], ref_nodes[first + 1] = (np.minimum(ref_nodes[first], ref_nodes[first + 1]),
                                                  np.maximum(ref_nodes[first], ref_nodes[first + 1]))
        np.testing.assert_array_equal(node_ptr, ref_ptr)
        np.testing.assert_array_equal(nodes, ref_nodes)
        np.testing.assert_array_equal(dists, ref_dists)
        ref, ptr, rn, _ = c_oracle.pos_rows(links.T, hops, A, X, K, plus=plus)
        np.testing.assert_array_equal(plan.row_ptr().cpu().numpy(), ptr)
        np.testing.assert_array_equal(plan.row_nodes().cpu().numpy(), rn)
        assert rel_err(rows.cpu().numpy(), ref) < TOL, (hops, K, mode)
        f.close()
    finally:
        plan.close()
    return node_ptr, dists


@pytest.mark.parametrize("hops", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("name", ["grid", "rand", "path", "ring"])
def test_structure_at_depth(eng, name, hops):
    """Node sets, dists and rows at hops 4..8, sign_k = hops (every level feeds an operator limit of the link
    kernels) and sign_k 3 (operators shallower than the subgraph)."""
    n, edges, links = GRAPHS[name]()
    A = csr_from_undirected(n, edges)
    G = eng.graph(A)
    for K, mode in ((hops, "pos_plus"), (3, "pos")):
        _check_structure(eng, G, A, links, hops, K, mode)
    G.close()


CSR_ROAD = {"S3GRL_FORCE_CSR", "S3GRL_NO_CSR"}
HOOKS = [("S3GRL_FORCE_HASH", "1"), ("S3GRL_NO_DM", "1"), ("S3GRL_LDS_BUDGET", "2048"),
         ("S3GRL_FORCE_EXT_BITMAPS", "1"), ("S3GRL_FORCE_CSR", "1"), ("S3GRL_NO_CSR", "1"),
         ("S3GRL_NO_RELABEL", "1"), ("S3GRL_STASH_SLOT", "16")]


@pytest.mark.parametrize("hook,value", HOOKS)
@pytest.mark.parametrize("name", ["grid", "rand", "ring"])
def test_structure_flavours_at_depth(eng, monkeypatch, name, hook, value):
    """One visited-set / class flavour per case (hash set, bitmap instead of the direct map, the HBM-scratch
    class, bitmaps in HBM slices, the CSR road and its absence, the caller's node order, overflowing stash
    slots) at hops 5 and 8 with sign_k below the depth, and at hops 4 and 7 with sign_k - 1 = hops: only there
    (every operator reaches the whole subgraph) may a plan take the induced-CSR road, which S3GRL_FORCE_CSR
    then sends every link down and S3GRL_NO_CSR none (class counts as in test_gpu_csr.py)."""
    monkeypatch.setenv(hook, value)
    n, edges, links = GRAPHS[name]()
    A = csr_from_undirected(n, edges)
    G = eng.graph(A)
    for hops, K in ((5, 5), (8, 6), (4, 5), (7, 8)):
        _check_structure(eng, G, A, links, hops, K)
        if hook in CSR_ROAD:
            cls = plan_classes(eng, G, eng.links(links.T.copy()), mode="pos_plus", num_hops=hops, sign_k=K,
                               full_stats=True)
            csr = hook == "S3GRL_FORCE_CSR" and K - 1 >= hops
            assert sum(cls[32:46]) == (len(links) if csr else 0), (hops, K, cls)
            if csr:
                assert sum(cls[:26]) == 0
    G.close()


@pytest.mark.parametrize("mode", ["pos", "pos_plus"])
def test_thirty_hops_on_a_path(eng, mode):
    """num_hops = 30 (the limit) with sign_k = 8 on an 80-node path: all 31 levels present; nodes, dists and
    rows exact against the oracle, the packed operand's element plan bit for bit with the chunk path."""
    import torch

    n, edges, links = path_graph()
    A = csr_from_undirected(n, edges)
    G = eng.graph(A)
    node_ptr, dists = _check_structure(eng, G, A, links, 30, 8, mode)
    for li in range(len(links)):
        assert set(dists[node_ptr[li]:node_ptr[li + 1]].tolist()) == set(range(31))
    X = operands(n, 5)["hi"]
    L = eng.links(links.T.copy())
    ref = c_oracle.pos_rows(links.T, 30, A, X, 8, plus=mode == "pos_plus")[0]
    out = {}
    for m in ("packed", "packed_only"):
        f = eng.features(X, m)
        out[m] = eng.precompute(G, f, L, mode=mode, num_hops=30, sign_k=8).rows
        f.close()
    assert torch.equal(out["packed"], out["packed_only"])
    assert_parity(out["packed"], A, links, 30, X, 8, mode == "pos_plus", ref)
    G.close()


def test_thirty_one_hops_refused(eng):
    from s3grl_amd.seal import enclosing_subgraphs

    n, edges, links = path_graph()
    A = csr_from_undirected(n, edges)
    G = eng.graph(A)
    L = eng.links(links.T.copy())
    f = eng.features(small_x(n))
    try:
        with pytest.raises(ValueError):
            eng.plan(G, L, mode="pos", num_hops=31, sign_k=3)
        with pytest.raises(ValueError):
            eng.precompute(G, f, L, mode="pos_plus", num_hops=31, sign_k=8)
        with pytest.raises(ValueError):
            enclosing_subgraphs(links.T, A, None, 1, 31, "drnl", engine=eng)
    finally:
        f.close()
        G.close()


@pytest.mark.parametrize("case", range(6))
def test_directed_and_sampled_at_depth(eng, case):
    """Directed grids (each edge one way, some both; hops follow out- and in-arcs) and per-hop sampling at
    hops 4..6, against the reference-structured Python oracle."""
    import scipy.sparse as ssp

    import oracle

    rng = np.random.default_rng(700 + case)
    n, edges, links = grid_graph(rows=10, cols=14, chords=4, seed=case)
    directed = case % 2 == 0
    sampled = case >= 3
    hops = 4 + case % 3
    K = [4, 5, 8, 3, 6, 7][case]
    plus = case % 3 != 1
    if directed:
        flip = rng.random(len(edges)) < 0.5
        arcs = np.where(flip[:, None], edges[:, ::-1], edges)
        both = edges[rng.random(len(edges)) < 0.3]
        arcs = np.unique(np.vstack([arcs, both[:, ::-1]]), axis=0)
        A = ssp.csr_matrix((np.ones(len(arcs), dtype=np.int64), (arcs[:, 0], arcs[:, 1])), shape=(n, n))
        A_csc = A.tocsc()
        G = eng.graph(A, directed=True, A_csc=A_csc)
        okw = {"directed": True, "A_csc": A_csc}
    else:
        A = csr_from_undirected(n, edges)
        G = eng.graph(A)
        okw = {}
    smp, osmp = {}, {}
    if sampled:
        smp = {"ratio_per_hop": 0.6, "max_nodes_per_hop": 12, "seed": case}
        osmp = {"ratio_per_hop": 0.6, "max_nodes_per_hop": 12, "sample_seed": case}
    X = (rng.standard_normal((n, 20)) * (rng.random((n, 20)) < 0.5)).astype(np.float32)
    res = eng.precompute(G, eng.features(X), eng.links(links.T.copy()), mode="pos_plus" if plus else "pos",
                         num_hops=hops, sign_k=K, **smp)
    kw = {"sign_k": K, "k_node_set_strategy": "intersection"}
    fn = oracle.get_PoS_Plus_prepped_ds if plus else oracle.get_PoS_prepped_ds
    ref, ptr, _ = oracle.collate_rows(fn(links.T, hops, A, X.astype(np.float64), 1, kw, dtype=np.float64,
                                         **okw, **osmp), K)
    np.testing.assert_array_equal(res.row_ptr.cpu().numpy(), ptr)
    err = rel_err(res.rows.cpu().numpy(), ref)
    if err >= TOL:      # cancellation of signed features?  judge against the sum of the absolute terms
        terms, _, _ = oracle.collate_rows(fn(links.T, hops, A, np.abs(X).astype(np.float64), 1, kw,
                                             dtype=np.float64, **okw, **osmp), K)
        err = rel_err(res.rows.cpu().numpy(), ref, terms)
    assert err < TOL, (case, hops, K, plus, err)
    G.close()


# ---- SEAL at depth --------------------------------------------------------------------------------------

@pytest.mark.parametrize("hops", [4, 6, 30])
@pytest.mark.parametrize("name", ["grid", "ring", "path", "fan"])
def test_seal_at_depth(eng, name, hops):
    """Labelled enclosing subgraphs: node lists and dists against c_oracle.extract, edges and every label
    against the test restatement (seal_reference.label_subgraph).  On the ring at hops 30 (the whole ring) the
    distances with one endpoint masked go the long way round, beyond the hop count; on the fan they go beyond
    2 * hops at every depth, and beyond DE+'s clamp at 100."""
    from seal_reference import LABELS, label_subgraph
    from s3grl_amd.seal import enclosing_subgraphs

    n, edges, links = GRAPHS[name]()
    A = csr_from_undirected(n, edges)
    ref_ptr, ref_nodes, ref_dists = c_oracle.extract(links.T, hops, A)
    longest, clamped = 0, 0
    for label in LABELS:
        s = enclosing_subgraphs(links.T, A, None, 1, hops, label, engine=eng).subs
        h = {k: getattr(s, k).cpu().numpy() for k in ("node_ptr", "nodes", "dists", "edge_ptr", "src", "dst",
                                                       "weight", "z")}
        np.testing.assert_array_equal(h["node_ptr"], ref_ptr)
        np.testing.assert_array_equal(h["nodes"], ref_nodes)
        np.testing.assert_array_equal(h["dists"], ref_dists)
        for i in range(len(links)):
            a, b = h["node_ptr"][i], h["node_ptr"][i + 1]
            c, d = h["edge_ptr"][i], h["edge_ptr"][i + 1]
            e = np.stack([h["src"][c:d], h["dst"][c:d], h["weight"][c:d]], 1).astype(np.int64)
            edges_ref, z_ref = label_subgraph(A, h["nodes"][a:b], h["dists"][a:b], label)
            np.testing.assert_array_equal(e, edges_ref, err_msg=f"link {i}")
            np.testing.assert_array_equal(h["z"][a:b], z_ref, err_msg=f"link {i} {label}")
            if label == "de+":
                longest = max(longest, int(np.max(np.where(z_ref < 100, z_ref, 0))))
                clamped += int(np.sum(z_ref == 100))
    if name == "ring" and hops == 30:
        assert longest == n - 2          # (0, 1) masked: from 0 to 2 the long way round, beyond the hop count
    if name == "fan":
        assert longest == 99 > 2 * hops and clamped > 0    # reached nodes 100 .. 150 steps away: clamped
