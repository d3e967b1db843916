"""CPU checks of the labelled enclosing subgraphs (SEAL baselines): the test restatement against the
reference-pinned fixtures, the new C ABI symbols, and the argument checks of s3grl_amd.seal (no GPU)."""
import re
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as ssp

from conftest import GOLDEN, csr_from_arcs, csr_from_undirected
from seal_reference import LABELS, label_subgraph, ragged, tag

REPO = Path(__file__).resolve().parent.parent
CASES = ["triangle", "pair", "star_iso", "probe5", "rand300", "usair", "cora", "directed_tiny", "directed_usair"]
NEW_SYMBOLS = ["s3grl_subgraphs_create", "s3grl_subgraphs_counts", "s3grl_subgraphs_export",
               "s3grl_subgraphs_destroy"]


def load_case(name):
    lab = np.load(GOLDEN / f"labels_{name}.npz")
    ext = np.load(GOLDEN / f"extract_{name}.npz")
    n = int(lab["num_nodes"])
    A = csr_from_arcs(n, lab["arcs"]) if int(lab["directed"]) else csr_from_undirected(n, lab["edges"])
    return lab, ext, A


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_reference_fixtures(name):
    lab, ext, A = load_case(name)
    for h in (int(x) for x in lab["hops"]):
        for li in range(len(lab["links"])):
            nodes = ragged(lab, f"h{h}_nodes", li)
            ext_nodes = ragged(ext, f"h{h}_nodes", li)        # (hop 0 in ascending id there)
            assert list(nodes[:2]) == list(lab["links"][li])
            np.testing.assert_array_equal(np.sort(nodes[:2]), ext_nodes[:2])
            np.testing.assert_array_equal(nodes[2:], ext_nodes[2:])
            dists = ragged(ext, f"h{h}_dists", li)
            exp_edges = ragged(lab, f"h{h}_edges", li).astype(np.int64)
            for label in LABELS:
                edges, z = label_subgraph(A, nodes, dists, label)
                np.testing.assert_array_equal(z, ragged(lab, f"h{h}_z_{tag(label)}", li),
                                              err_msg=f"{name} h={h} link {li} {label}")
                if label == "drnl":
                    g = np.stack([nodes[edges[:, 0]], nodes[edges[:, 1]], edges[:, 2]], 1) if len(edges) \
                        else edges
                    g = g[np.lexsort((g[:, 1], g[:, 0]))]
                    np.testing.assert_array_equal(g, exp_edges)


def test_fixtures_pin_the_de_and_drnl_quirks():
    """A negative link's endpoints are at distance 1 under `de` (the explicit zero of the target entry counts
    as an edge), unreached nodes get 3, never 4; DRNL gives 0 to a node one endpoint cannot reach."""
    lab, ext, A = load_case("star_iso")
    links = [tuple(int(v) for v in l) for l in lab["links"]]
    li = links.index((0, 6))                   # 6 is isolated: a negative link
    z = ragged(lab, "h2_z_de", li)
    np.testing.assert_array_equal(z[:2], [[0, 1], [1, 0]])
    assert z.max() <= 3
    zd = ragged(lab, "h2_z_drnl", li)
    assert (zd[2:] == 0).all() and zd[0] == 1 and zd[1] == 1
    zp = ragged(lab, "h2_z_deplus", li)
    np.testing.assert_array_equal(zp[:2], [[0, 0], [0, 0]])
    assert (zp[2:, 1] == 100).all()


def test_header_and_library_export_the_subgraph_calls():
    import __graft_entry__ as ge

    ge.build()
    from s3grl_amd import _native

    header = (REPO / "include" / "s3grl.h").read_text()
    declared = set(re.findall(r"\b(s3grl_[a-z_]+)\s*\(", header))
    lib = _native.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name) is not None


def test_argument_checks_need_no_gpu():
    from s3grl_amd import enclosing_subgraphs
    from s3grl_amd.seal import label_code

    A = csr_from_undirected(5, [[0, 1], [1, 2], [2, 3], [3, 4]])
    ok = np.array([[0, 2], [1, 3]])
    with pytest.raises(ValueError):
        enclosing_subgraphs(np.array([0, 1]), A, None, 1, 2)                   # not [2, L]
    with pytest.raises(ValueError):
        enclosing_subgraphs(np.array([[0], [5]]), A, None, 1, 2)               # endpoint outside [0, N)
    with pytest.raises(ValueError):
        enclosing_subgraphs(np.array([[-1], [2]]), A, None, 1, 2)
    with pytest.raises(ValueError):
        enclosing_subgraphs(np.array([[3], [3]]), A, None, 1, 2)               # src == dst
    with pytest.raises(ValueError):
        enclosing_subgraphs(ok, A, None, 1, 0)                                 # num_hops
    with pytest.raises(ValueError):
        enclosing_subgraphs(ok, A, None, 1, 2, ratio_per_hop=0.0)
    with pytest.raises(ValueError):
        enclosing_subgraphs(ok, A, None, 1, 2, max_nodes_per_hop=0)
    with pytest.raises(ValueError):
        enclosing_subgraphs(ok, A[:, :4], None, 1, 2)                          # not square
    with pytest.raises(ValueError):
        enclosing_subgraphs(ok, A, np.zeros((4, 3)), 1, 2)                     # x rows
    with pytest.raises(ValueError):
        enclosing_subgraphs(ok, ssp.csr_matrix(A.toarray()).toarray(), None, 1, 2)   # dense A
    assert [label_code(l) for l in ["drnl", "de", "de+", "hop", "zo", "degree"]] == [0, 1, 2, 3, 4, 5]
    assert label_code("cn") == label_code("") == 6                            # anything else: zeros
