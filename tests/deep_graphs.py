"""Test infrastructure: the generated graphs of the deep-subgraph tests, shared by the GPU file
(test_gpu_deep_hops.py) and the host cross-check of the two restatements (test_oracle_c.py).

Each builder returns (n, undirected edges [e, 2], links [L, 2]), all from seeded numpy (rand300: the
committed extraction fixture)."""
import numpy as np

from conftest import load_extract


def grid_graph(rows=12, cols=25, chords=6, seed=0):
    """A rows x cols grid plus `chords` random long edges; links around the centre (edges, non-edges,
    reversed duplicates and a repeat), and two on row 0, where the feature matrices of the gather tests keep
    their long rows (nodes 7, 11 and 13 of the default grid): (7, 13) has two of them as endpoints and the
    third two hops away, (11, 36) the empty one as an endpoint, so every depth gathers them."""
    rng = np.random.default_rng(seed)
    idx = np.arange(rows * cols).reshape(rows, cols)
    e = [np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()], 1), np.stack([idx[:-1].ravel(), idx[1:].ravel()], 1)]
    e.append(rng.integers(0, rows * cols, size=(chords, 2)))
    e = np.concatenate(e)
    e = np.unique(np.sort(e[e[:, 0] != e[:, 1]], axis=1), axis=0)
    r, c = rows // 2, cols // 2
    links = [(idx[r, c], idx[r, c + 1]), (idx[r, c - 3], idx[r + 1, c + 2]), (idx[r - 2, c], idx[r + 2, c + 4]),
             (idx[1, 2], idx[2, 2]), (idx[r, 0], idx[r, 5]), (idx[3, c + 6], idx[r + 3, c - 5]),
             (idx[0, 7], idx[0, 13]), (idx[0, 11], idx[1, 11])]
    links = links + [links[0][::-1], links[2][::-1], links[1]]
    return rows * cols, e, np.array(links, dtype=np.int64)


def rand_graph():
    g = load_extract("rand300")
    links = g["links"][:12]
    return int(g["num_nodes"]), g["edges"], np.concatenate([links, links[:3, ::-1], links[:2]])


def path_graph(n=80):
    e = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    m = n // 2
    links = np.array([(m - 1, m), (m - 2, m + 1), (m, m + 3), (m + 1, m - 1), (m, m - 1)], dtype=np.int64)
    return n, e, links


def ring_graph(n=40):
    e = np.stack([np.arange(n), (np.arange(n) + 1) % n], 1)
    links = np.array([(0, 1), (5, 7), (10, 30), (22, 21), (3, 12)], dtype=np.int64)
    return n, e, links


def fan_graph(m=150):
    """src 0 and dst 1 joined; dst joined to every node of the path 2 .. m + 1, src to its first node.  Every
    node is within one hop, yet with dst masked src reaches node m + 1 only along the path, in m steps."""
    path = np.arange(2, m + 2)
    e = np.concatenate([[(0, 1), (0, 2)], np.stack([np.ones(m, np.int64), path], 1),
                        np.stack([path[:-1], path[1:]], 1)])
    links = np.array([(0, 1), (1, 0), (2, 1), (0, m + 1)], dtype=np.int64)
    return m + 2, e, links


GRAPHS = {"grid": grid_graph, "rand": rand_graph, "path": path_graph, "ring": ring_graph, "fan": fan_graph}


