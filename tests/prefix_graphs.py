"""Test infrastructure: "broom" graphs whose hop sizes are set by construction, for the tests of the packed
gather's prefix schedule (test_gpu_gather_prefix.py on the GPU, test_gather_prefix_host.py for the sizes).

A broom is one link (src, dst) with n1 nodes at hop 1, n2 at hop 2 and n3 at hop 3: the hop-1 nodes hang on src
(the last of them on dst as well: a common neighbour, so PoS Plus has a second row pair), the hop-2 nodes on
the first hop-1 node, the hop-3 nodes on the first hop-2 node.  Every other broom also has the edge (src, dst),
which the operators mask.  The brooms of a table are disjoint components of one graph, one link each.

With sign_k = 3 and num_hops = 3 the gather's prefix (the rows the leading operators reach, list positions below
lim[K-2]) is the 2 + n1 + n2 nodes within two hops and the list has 2 + n1 + n2 + n3 rows; with sign_k = 2 the
prefix is the 2 + n1 nodes within one hop of a list that ends at hop 2."""
import numpy as np

W = 64   # kPrefixWindow of s3grl_amd/csrc/s3grl_packed.hip: rows per staged window of pass2
U = 4    # rows per group of the gather kernels
SEG = 16  # rows per piece when the split tests set S3GRL_SPLIT_SEG_SHIFT=4

# A list always starts with its two endpoints and a hop beyond the prefix needs a node in every hop before it:
# with a last hop beyond it the shortest prefix is 3 rows at sign_k = 2 and 4 at sign_k = 3.  Prefixes of 1, 2
# and 3 rows exist as the prefix of a PIECE: a list gathered in pieces of SEG rows hands every piece the part
# of the prefix that falls into it (lengths SEG + 1, SEG + 2, SEG + 3 below).
PREFIX_LENGTHS = [4, 5, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W + 2]
PIECE_PREFIX_LENGTHS = [1, 2, 3]           # as SEG + 1, SEG + 2, SEG + 3
SIGN_K2_PREFIX_LENGTHS = [3, W, W + 1, 2 * W + 1]

# (n1, n2, n3); prefix at sign_k = 3: 2 + n1 + n2
SHAPES = [
    (1, 1, 11),      # 4
    (1, 2, 11),      # 5
    (5, 10, 40),     # 17: one row into the second piece of a 57-row list
    (6, 10, 40),     # 18
    (7, 10, 40),     # 19
    (30, 31, 11),    # W - 1
    (31, 31, 11),    # W
    (31, 32, 11),    # W + 1
    (63, 62, 11),    # 2 W - 1   (sign_k = 2: W + 1)
    (61, 65, 11),    # 2 W
    (62, 65, 11),    # 2 W + 1   (sign_k = 2: W)
    (127, 65, 11),   # 3 W + 2   (sign_k = 2: 2 W + 1)
    (2, 2, 1),       # prefix 6 of a 7-row list: ends inside phase A (the prefix reaches into the last, partial group)
    (31, 32, 1),     # the same at a window's edge: prefix W + 1 of W + 2 rows
    (3, 3, 2),       # prefix 8 of 10 rows: the list ends two rows after phase A
    (31, 31, 3),     # prefix W of W + 3 rows: three rows after it
    (3, 3, 1),       # prefix 8 of 9 rows: one row after it
    (1, 9, 11),      # 12  (sign_k = 2: 3, the shortest prefix with a hop beyond it)
]
ENDS_INSIDE_A = [12, 13]      # indices into SHAPES
ENDS_AFTER_A = {16: 1, 14: 2, 15: 3}   # index -> rows after phase A


def brooms(shapes=SHAPES, reversed_links=False):
    """(n, undirected edges [e, 2], links [L, 2]) of the table's brooms; with `reversed_links` every link is
    followed by its reversed duplicate."""
    edges, links = [], []
    off = 0
    for i, (n1, n2, n3) in enumerate(shapes):
        src, dst = off, off + 1
        h1 = np.arange(off + 2, off + 2 + n1)
        h2 = np.arange(h1[-1] + 1, h1[-1] + 1 + n2)
        h3 = np.arange(h2[-1] + 1, h2[-1] + 1 + n3)
        e = [(src, v) for v in h1] + [(dst, h1[-1])] + [(h1[0], v) for v in h2] + [(h2[0], v) for v in h3]
        if i % 2 == 0:
            e.append((src, dst))
        edges += e
        links.append((src, dst))
        if reversed_links:
            links.append((dst, src))
        off = h3[-1] + 1
    return int(off), np.array(edges, dtype=np.int64), np.array(links, dtype=np.int64)


def hop_lists(n, edges, link):
    """numpy BFS from {src, dst} with the link itself masked: the nodes of hop 0, 1, 2, ... (ascending ids)."""
    adj = [[] for _ in range(n)]
    s, d = int(link[0]), int(link[1])
    for a, b in edges:
        a, b = int(a), int(b)
        if {a, b} == {s, d}:
            continue
        adj[a].append(b)
        adj[b].append(a)
    seen = np.zeros(n, dtype=bool)
    seen[[s, d]] = True
    hops = [np.array(sorted({s, d}), dtype=np.int64)]
    while True:
        nxt = sorted({v for u in hops[-1] for v in adj[u] if not seen[v]})
        if not nxt:
            return hops
        seen[nxt] = True
        hops.append(np.array(nxt, dtype=np.int64))


def phase_a_rows(prefix, cnt):
    """Rows of a cnt-row list that the gather's phase A covers for a prefix of `prefix` rows (groups of U rows;
    a prefix that reaches into the last, partial group takes the whole list), and whether it does so because
    the list ends inside phase A."""
    full = cnt // U * U
    if prefix > full:
        return cnt, True
    return min(full, (prefix + U - 1) // U * U), False
