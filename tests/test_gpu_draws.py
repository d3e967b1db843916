"""The draws of the trainers' shared generator (csrc/s3grl_train.hpp, s3grl_train.hip), pinned: what the export hooks
of MF, SIGNNet and node2vec hand out at (epoch, step) against the numpy restatement (tests/draws_reference.py), integer
for integer.  The shapes are the smallest at which the generator can go wrong: permutations of 1, 2, 257 (one past a
block) and 1025 elements, steps 0 and 1 of epochs 0 and 3 (the step / stream packing at both field widths), 3 nodes for
the negatives, dropout 0, 0.5 and 1 - 2^-33 (the threshold clamps to 2^32 - 1), a hidden width that is no multiple of
the lanes per pair.  The float initial values are not pinned: logf and cosf may move with the compiler."""
import numpy as np
import pytest
import torch

import draws_reference as D

SEED = 0x9e3779b9                     # bit 31 set: the seed is taken as an unsigned 32-bit value
EPOCHS, STEPS = (0, 3), (0, 1)
CLAMPED = 1.0 - 2.0 ** -33            # p · 2^32 = 2^32 - 0.5: above the largest threshold
DROPOUTS = (0.0, 0.5, CLAMPED)


def _np(t):
    return t.cpu().numpy()


def test_restatement_and_build_list():
    """Host only: the unit is built, and the restatement's own edge cases."""
    assert "s3grl_train.hip" in __import__("__graft_entry__").SOURCES
    assert D.drop_below(0.0) == 0 and D.drop_below(0.5) == 1 << 31
    assert D.drop_below(CLAMPED) == (1 << 32) - 1 > D.drop_below(0.999999)
    assert D.stream_key(1, 2, 1, 0, 2) == D.stream_key(1, 2, 0, 4, 3) != D.stream_key(1, 2, 1, 0, 3)
    for n in (1, 2, 257):
        assert sorted(D.permutation(D.stream_key(SEED, 0, 0, 2, 3), n)) == list(range(n))
    assert int(D.below(0xffffffff, 3)) == 2 and int(D.below(0, 3)) == 0
    assert D.keep_mask(5, 4, 7, 0.0).all() and not D.keep_mask(5, 64, 64, CLAMPED).any()


@pytest.mark.gpu
@pytest.mark.parametrize("p", DROPOUTS)
def test_mf_draws(p):
    from s3grl_amd.mf import MFTrainer

    n, H, L = 3, 5, 3                                                   # 5 channels on 8 lanes per pair
    mf = MFTrainer(n, H, L, p, 0.01, seed=SEED)
    for E, bs in ((1, 32), (2, 32), (257, 128), (1025, 1024)):
        for epoch in EPOCHS:
            for step in STEPS:
                if step * bs >= E:
                    continue
                idx, neg, masks = (_np(t) for t in mf.draws(epoch, step, E, bs))
                ridx, rneg, rmasks = D.mf_draws(SEED, epoch, step, E, bs, n, L, H, p)
                what = f"E={E} epoch={epoch} step={step}"
                np.testing.assert_array_equal(idx, ridx, err_msg=what)
                np.testing.assert_array_equal(neg, rneg, err_msg=what)
                np.testing.assert_array_equal(masks, rmasks, err_msg=what)
                assert p > 0.0 or masks.all()                           # dropout 0 keeps everything
    mf.close()


@pytest.mark.gpu
@pytest.mark.parametrize("p", DROPOUTS)
def test_signnet_draws(p):
    from s3grl_amd.signnet import SIGNNetTrainer

    H = 6                                                               # no multiple of the 4 columns of a slice
    net = SIGNNetTrainer(4, hidden=H, dropout=p, seed=SEED)
    for L, B in ((2, 2), (257, 64), (1025, 64)):
        row_ptr = np.concatenate([[0], np.cumsum(2 + np.arange(L) % 3)])
        for epoch in EPOCHS:
            for step in STEPS:
                if step * B >= L - 1:
                    continue
                ids, mask1, mask2 = (_np(t) for t in net.draws(epoch, step, L, B, row_ptr=torch.as_tensor(row_ptr)))
                rids, rmask1, rmask2 = D.signnet_draws(SEED, epoch, step, L, B, row_ptr, H, p)
                what = f"L={L} epoch={epoch} step={step}"
                np.testing.assert_array_equal(ids, rids, err_msg=what)
                np.testing.assert_array_equal(mask1, rmask1, err_msg=what)
                np.testing.assert_array_equal(mask2, rmask2, err_msg=what)
    net.close()


# N = 3: the negatives; a 5-node path, every degree known: the positives; 257 nodes without an edge: a permutation one
# past a block at the 2-bit width (every row stays on its start node)
PATH5 = np.array([[0, 1, 1, 2, 2, 3, 3, 4], [1, 0, 2, 1, 3, 2, 4, 3]])
N2V_GRAPHS = {"n3": (3, np.array([[0, 1, 1, 2], [1, 0, 2, 1]]), 2), "path5": (5, PATH5, 2),
              "isolated257": (257, np.zeros((2, 0), dtype=np.int64), 256)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(N2V_GRAPHS))
def test_node2vec_windows(name):
    from s3grl_amd.node2vec import Node2Vec, csr_of

    n, edges, bs = N2V_GRAPHS[name]
    walk, ctx, R, Q = 4, 3, 2, 2
    m = Node2Vec(edges, n, 4, walk_length=walk, context_size=ctx, walks_per_node=R, num_negative_samples=Q, seed=SEED)
    indptr, indices = csr_of(edges, n)
    for epoch in EPOCHS:
        for step in STEPS:
            pos, neg = (_np(t) for t in m.windows(epoch, step, bs))
            rpos, rneg = D.n2v_windows(SEED, epoch, step, bs, indptr, indices.astype(np.int64), walk, ctx, R, Q)
            np.testing.assert_array_equal(neg, rneg, err_msg=f"{name} epoch={epoch} step={step}")
            np.testing.assert_array_equal(pos, rpos, err_msg=f"{name} epoch={epoch} step={step}")
    m.close()
