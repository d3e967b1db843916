"""The structure builder of s3grl_amd.propagate on CPU tensors against a few lines of plain numpy: ptr_of, csr_both, the
add_remaining_self_loops step and the raw operator's scale, on a 12-node directed graph with a duplicated arc, two input
self-loops (one with a weight of its own), a node without in-arcs (0) and a node without any arc (11)."""
import numpy as np
import torch

N_NODES = 12
#          duplicated: 3 -> 5 twice          loops: (2, 2) and (7, 7)
ARCS = [(0, 1), (3, 5), (0, 2), (2, 2), (3, 5), (1, 5), (4, 3), (7, 7), (5, 4), (6, 7), (0, 6), (8, 9), (9, 10), (10, 8),
        (9, 1), (4, 9)]
WEIGHT = [10.0 + k for k in range(len(ARCS))]       # distinct, so that an entry names its arc
WEIGHT[3] = 2.5                                     # the loop of node 2; the loop of node 7 keeps 17


def _tensors():
    a = np.asarray(ARCS, dtype=np.int64)
    return torch.as_tensor(a[:, 0].copy()), torch.as_tensor(a[:, 1].copy()), torch.tensor(WEIGHT, dtype=torch.float64)


def _rows(arcs, key, other):
    """Per node, the arcs (by input position) whose `key` end it is, ordered by the `other` end, then input position."""
    return [sorted((k for k, a in enumerate(arcs) if a[key] == i), key=lambda k: (arcs[k][other], k))
            for i in range(N_NODES)]


def test_graph_has_the_cases():
    src, dst = np.asarray(ARCS).T
    indeg, outdeg = np.bincount(dst, minlength=N_NODES), np.bincount(src, minlength=N_NODES)
    assert len(set(ARCS)) == len(ARCS) - 1 and ARCS.count((3, 5)) == 2
    assert [a for a in ARCS if a[0] == a[1]] == [(2, 2), (7, 7)]
    assert indeg[0] == 0 and outdeg[0] > 0
    assert indeg[11] == 0 and outdeg[11] == 0


def test_ptr_of():
    from s3grl_amd.propagate import ptr_of

    _, dst, _ = _tensors()
    want = [int((dst.numpy() < i).sum()) for i in range(N_NODES + 1)]
    got = ptr_of(dst, N_NODES)
    assert got.dtype == torch.int64 and got.tolist() == want
    assert ptr_of(dst[:0], 3).tolist() == [0, 0, 0, 0]


def test_csr_both_lists_every_arc_once_duplicates_in_input_order():
    from s3grl_amd.propagate import csr_both

    src, dst, _ = _tensors()
    shift = torch.arange(N_NODES, dtype=torch.int32) + 100          # any map from a node to its neighbour id
    in_ptr, in_nbr, perm_in, out_ptr, out_nbr, perm_out = csr_both(src, dst, N_NODES, lambda ids: shift[ids])
    for ptr, nbr, perm, key, other in ((in_ptr, in_nbr, perm_in, 1, 0), (out_ptr, out_nbr, perm_out, 0, 1)):
        rows = _rows(ARCS, key, other)
        assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in rows])]).tolist()
        assert perm.tolist() == [k for r in rows for k in r]
        assert sorted(perm.tolist()) == list(range(len(ARCS)))      # every arc exactly once
        assert nbr.dtype == torch.int32 and nbr.is_contiguous()
        assert nbr.tolist() == [100 + ARCS[k][other] for r in rows for k in r]
    a = in_ptr[5]
    assert perm_in[a:a + 3].tolist() == [5, 1, 4]                   # 1 -> 5, then 3 -> 5 twice, in input order
    b = out_ptr[3]
    assert perm_out[b:b + 2].tolist() == [1, 4]


def test_add_remaining_self_loops():
    from s3grl_amd.propagate import add_remaining_self_loops

    src, dst, w = _tensors()
    keep = [k for k, (s, d) in enumerate(ARCS) if s != d]
    want_src = [ARCS[k][0] for k in keep] + list(range(N_NODES))
    want_dst = [ARCS[k][1] for k in keep] + list(range(N_NODES))
    loop_w = np.ones(N_NODES, dtype=np.float32)
    for k, (s, d) in enumerate(ARCS):
        if s == d:
            loop_w[s] = WEIGHT[k]
    assert loop_w[2] == 2.5 and loop_w[7] == 17.0 and (np.delete(loop_w, [2, 7]) == 1).all()
    s2, d2, w2 = add_remaining_self_loops(src, dst, w, N_NODES)
    assert s2.tolist() == want_src and d2.tolist() == want_dst
    assert w2.dtype == torch.float32
    assert w2.tolist() == [WEIGHT[k] for k in keep] + loop_w.tolist()
    s3, d3, w3 = add_remaining_self_loops(src, dst, None, N_NODES)
    assert s3.tolist() == want_src and d3.tolist() == want_dst and w3 is None


def test_raw_operator_keeps_the_list_and_scales_by_in_degree():
    from s3grl_amd.propagate import _RawOperator

    src, dst, _ = _tensors()
    loc = torch.arange(N_NODES, dtype=torch.int32)
    op = _RawOperator()
    op._build(src, dst, None, loc, N_NODES)
    indeg = np.bincount(dst.numpy(), minlength=N_NODES)
    assert op.in_nbr.numel() == op.out_nbr.numel() == len(ARCS)      # loops and duplicates are edges
    assert op.in_ptr.diff().tolist() == indeg.tolist()
    assert op.scale.dtype == torch.float32
    assert op.scale.tolist() == (np.float32(1) / np.maximum(indeg, 1).astype(np.float32)).tolist()
    assert op.scale[0] == 1 and op.scale[11] == 1 and op.scale[5] == np.float32(1) / np.float32(3)
    assert op.num_nodes == N_NODES and op.loc is loc
