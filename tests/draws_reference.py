"""The trainers' draw generator (csrc/s3grl_train.hpp) restated on numpy uint64 arrays: the stream key at both field
widths, the 32-bit draw, the range reduction, the epoch permutation and the dropout mask rule; and, on top of them, what
each trainer's export hook hands out at (epoch, step).  Integer arithmetic only: every value is exact."""
import numpy as np

from gae_reference import mix64

U = np.uint64
# the stream numbers and the width of the stream field under the step: part of every draw
N2V = dict(bits=2, pos_walk=0, neg_draw=1, permute=2)
MF = dict(bits=3, neg_pair=0, mask=1, permute=2)
SIGNNET = dict(bits=3, mask1=0, mask2=1, permute=2)


def stream_key(seed, epoch, step, stream, bits):
    """mix64(mix64(mix64(seed) ^ epoch) ^ (step << bits | stream)) as a Python int."""
    assert 0 <= stream < 1 << bits
    k = int(mix64([seed & 0xffffffff])[0]) ^ epoch
    k = int(mix64([k])[0]) ^ ((step << bits) | stream)
    return int(mix64([k & 0xffffffffffffffff])[0])


def draw(key, row, pos):
    """32 random bits for every (row, position) of one stream; row and pos broadcast."""
    row, pos = np.asarray(row, dtype=U), np.asarray(pos, dtype=U)
    return mix64(U(key) ^ mix64((row << U(32)) ^ pos)) >> U(32)


def below(r, n):
    """floor(r · n / 2^32): a 32-bit draw onto [0, n), n < 2^32 (n broadcasts)."""
    return (np.asarray(r, dtype=U) * np.asarray(n, dtype=U)) >> U(32)


def permutation(key, n):
    """The epoch's permutation of range(n): the argsort of (draw(key, 0, i) << 32 | i), whose keys are distinct."""
    i = np.arange(n, dtype=U)
    return np.argsort((draw(key, 0, i) << U(32)) | i, kind="stable").astype(np.int64)


def drop_below(p):
    """An element is dropped when its draw is below this: min(p · 2^32, 2^32 − 1), truncated."""
    return int(min(p * 4294967296.0, 4294967295.0))


def keep_mask(key, rows, cols, p):
    """uint8 [rows, cols]: 1 where element (row, col) draws at or above the threshold."""
    d = draw(key, np.arange(rows, dtype=U)[:, None], np.arange(cols, dtype=U)[None, :])
    return (d >= U(drop_below(p))).astype(np.uint8)


# ---- what the hooks export ---------------------------------------------------------------------------------------
def mf_draws(seed, epoch, step, num_train, batch_size, num_nodes, num_layers, hidden, p):
    """MFTrainer.draws: pos_idx [B], neg [B, 2], masks uint8 [2B, num_layers − 1, hidden]."""
    B = min(batch_size, num_train - step * batch_size)
    perm = permutation(stream_key(seed, epoch, 0, MF["permute"], MF["bits"]), num_train)
    kneg = stream_key(seed, epoch, step, MF["neg_pair"], MF["bits"])
    neg = below(draw(kneg, np.arange(B, dtype=U)[:, None], np.arange(2, dtype=U)[None, :]), num_nodes)
    kmask = stream_key(seed, epoch, step, MF["mask"], MF["bits"])
    masks = keep_mask(kmask, 2 * B, (num_layers - 1) * hidden, p).reshape(2 * B, num_layers - 1, hidden)
    return perm[step * batch_size:step * batch_size + B], neg.astype(np.int64), masks


def signnet_draws(seed, epoch, step, num_links, batch_size, row_ptr, hidden, p):
    """SIGNNetTrainer.draws: ids [b], mask1 uint8 [ΣR_b, hidden] (a row per row of the batch), mask2 uint8 [b, hidden]."""
    b = min(batch_size, num_links - step * batch_size)
    perm = permutation(stream_key(seed, epoch, 0, SIGNNET["permute"], SIGNNET["bits"]), num_links)
    ids = perm[step * batch_size:step * batch_size + b]
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    rows = int((row_ptr[ids + 1] - row_ptr[ids]).sum())
    mask1 = keep_mask(stream_key(seed, epoch, step, SIGNNET["mask1"], SIGNNET["bits"]), rows, hidden, p)
    mask2 = keep_mask(stream_key(seed, epoch, step, SIGNNET["mask2"], SIGNNET["bits"]), b, hidden, p)
    return ids, mask1, mask2


def n2v_windows(seed, epoch, step, batch_size, indptr, indices, walk_length, context_size, walks_per_node,
                num_negative_samples):
    """Node2Vec.windows: (pos [W·B·R, C], neg [W·B·R·Q, C]), window-index-major.  Row r starts at batch[r % B]; a
    positive row walks uniformly over the CSR entries of its node (a node without entries stays put), a negative row
    draws every further node from [0, N)."""
    n = len(indptr) - 1
    B = min(batch_size, n - step * batch_size)
    perm = permutation(stream_key(seed, epoch, 0, N2V["permute"], N2V["bits"]), n)
    batch = perm[step * batch_size:step * batch_size + B]
    kpos = stream_key(seed, epoch, step, N2V["pos_walk"], N2V["bits"])
    kneg = stream_key(seed, epoch, step, N2V["neg_draw"], N2V["bits"])
    W, C = walk_length + 2 - context_size, context_size

    def windows(walks):                                   # [rows, walk_length + 1] -> [W · rows, C]
        return np.concatenate([walks[:, j:j + C] for j in range(W)])

    rp = B * walks_per_node
    pos = np.empty((rp, walk_length + 1), dtype=np.int64)
    pos[:, 0] = batch[np.arange(rp) % B]
    for s in range(1, walk_length + 1):
        cur = pos[:, s - 1]
        deg = indptr[cur + 1] - indptr[cur]
        pick = below(draw(kpos, np.arange(rp, dtype=U), s), deg).astype(np.int64)
        at = np.minimum(indptr[cur] + pick, len(indices) - 1)      # (a node without entries: any valid index)
        pos[:, s] = np.where(deg > 0, indices[at], cur) if len(indices) else cur
    rn = rp * num_negative_samples
    neg = np.empty((rn, walk_length + 1), dtype=np.int64)
    neg[:, 0] = batch[np.arange(rn) % B]
    neg[:, 1:] = below(draw(kneg, np.arange(rn, dtype=U)[:, None], np.arange(1, walk_length + 1, dtype=U)[None, :]), n)
    return windows(pos), windows(neg)
