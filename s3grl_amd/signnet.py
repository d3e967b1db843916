"""SIGNNet, the model that consumes the engine's rows (reference models.py:301-383; twin `harness.SIGNNetTwin`), trained
by fused HIP kernels behind the C ABI (s3grl_signnet_*, csrc/s3grl_signnet.hip): a mini-batch step is four launches on
the engine's stream instead of the several dozen of the eager loop in `harness.train_and_evaluate`.

    res = eng.precompute(g, x, links, mode="pos", num_hops=1, sign_k=3)            # rows [ΣR, K+1, 1+F], row_ptr [L+1]
    net = SIGNNetTrainer(res.rows.shape[1] * res.rows.shape[2], hidden=256, lr=1e-4, seed=1)
    losses = net.fit_epoch(res.rows, res.row_ptr, y, batch_size=32)                # one wait per epoch
    logits = net.score(test.rows, test.row_ptr)                                    # eval mode, fp32 [L]
    twin = SIGNNetTwin(in_width, 256); twin.load_state_dict(net.state_dict())      # and back: init=twin.state_dict()

Same semantics as the twin: operator_diff = Linear, ELU, BatchNorm1d (batch statistics over the ΣR_b rows of the batch,
running statistics with momentum 0.1 and the unbiased variance), dropout; centre pooling exactly as
`pool.centre_pool`; link_pred_mlp = Linear, ReLU, BatchNorm1d over the B links, dropout, Linear; BCE with logits; one
dense `torch.optim.Adam` step over the ten tensors.  A link's rows are read in place from the row store: there is no
`rows[idx]` copy.  Initial values are torch's distributions; the epoch's permutation and both dropout masks come from
the engine's counter-based generator keyed by (seed, epoch, step, stream, index): torch's distributions, NOT its random
streams.  Two runs with one seed are bit-identical.  GPU only; no CPU fallback.  `k_pool_strategy="concat"` stays on the
torch twin (NotImplementedError here), as do hidden > 256, in_width > 2^20 and batches of more than 64 links.

`SIGNNetRuns` trains the runs of a config (the reference's `for run in range(args.runs)`) side by side: up to 16
trainers that differ in seed (and dropout, lr) take every step of an epoch in the same four launches, each bit-identical
to the lone trainer of its seed.

    runs = SIGNNetRuns(in_width, hidden=256, lr=1e-4, seeds=range(10))
    losses = runs.fit_epoch(res.rows, res.row_ptr, y, batch_size=32)               # fp32 [10, steps]
    logits = runs.score(test.rows, test.row_ptr)                                   # fp32 [10, L]
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N

# SIGNNetTwin's state_dict keys of the ten trained tensors, in the engine's packing order, then the buffers
PARAM_KEYS = ("operator_diff.0.weight", "operator_diff.0.bias", "operator_diff.2.weight", "operator_diff.2.bias",
              "link_pred_mlp.0.weight", "link_pred_mlp.0.bias", "link_pred_mlp.2.weight", "link_pred_mlp.2.bias",
              "link_pred_mlp.4.weight", "link_pred_mlp.4.bias")
STAT_KEYS = ("operator_diff.2.running_mean", "operator_diff.2.running_var", "link_pred_mlp.2.running_mean",
             "link_pred_mlp.2.running_var")
COUNT_KEYS = ("operator_diff.2.num_batches_tracked", "link_pred_mlp.2.num_batches_tracked")
# the order of `SIGNNetTwin.state_dict()`
STATE_ORDER = PARAM_KEYS[:4] + STAT_KEYS[:2] + COUNT_KEYS[:1] + PARAM_KEYS[4:8] + STAT_KEYS[2:] + COUNT_KEYS[1:] + \
    PARAM_KEYS[8:]


def _pool_mode(k_heuristic, k_pool_strategy):
    if not k_heuristic:
        return 0
    if k_pool_strategy == "concat":
        raise NotImplementedError('k_pool_strategy="concat" is not fused: train it with harness.SIGNNetTwin')
    if k_pool_strategy not in ("mean", "sum"):
        raise NotImplementedError(f"Check pool strat: only mean / sum are fused, got {k_pool_strategy!r}")
    return N.SIGNNET_POOL[k_pool_strategy]


def _check_shape(hidden, in_width, batch=2):
    if hidden < 1 or in_width < 1:
        raise ValueError(f"need hidden >= 1 and in_width >= 1, got {hidden} and {in_width}")
    if batch < 2:
        raise ValueError(f"a training batch needs two links or more (BatchNorm), got {batch}")
    if hidden > N.SIGNNET_MAX_HIDDEN:
        raise NotImplementedError(f"SIGNNet with hidden above {N.SIGNNET_MAX_HIDDEN}, got {hidden}")
    if in_width > N.SIGNNET_MAX_WIDTH:
        raise NotImplementedError(f"SIGNNet with in_width above {N.SIGNNET_MAX_WIDTH}, got {in_width}")
    if batch > N.SIGNNET_MAX_BATCH:
        raise NotImplementedError(f"SIGNNet with batch_size above {N.SIGNNET_MAX_BATCH}, got {batch}")


def layout(hidden, in_width, batch, pooled=False):
    """The layout of the step kernels, without a GPU: dict(columns_per_workgroup, workgroups, rows_per_wave, k_vector,
    k_tile, head_k_vector, row_tile, score_tile).  Every launch is `workgroups` column slices of columns_per_workgroup
    hidden columns; a wavefront carries rows_per_wave rows per pass over in_width, its lanes k_vector floats per load
    (k_tile = 64 · k_vector per pass; head_k_vector along the head's ch · hidden inputs, ch = 2 when `pooled`); the dW1
    pass takes the batch's rows in tiles of row_tile and `score` the links in tiles of score_tile."""
    hidden, in_width, batch = int(hidden), int(in_width), int(batch)
    _check_shape(hidden, in_width, batch)
    out = (C.c_int32 * 8)()
    N.check(N.lib().s3grl_signnet_layout(hidden, in_width, batch, int(bool(pooled)), out), "s3grl_signnet_layout")
    keys = ("columns_per_workgroup", "workgroups", "rows_per_wave", "k_vector", "k_tile", "head_k_vector", "row_tile",
            "score_tile")
    return dict(zip(keys, out))


def _link_ids(ids, num_links, what="link_ids"):
    """Integer link ids in [0, num_links) -> int64 CPU tensor [B]."""
    t = ids if isinstance(ids, torch.Tensor) else torch.as_tensor(np.asarray(ids))
    if t.dim() != 1:
        raise ValueError(f"{what} must be [B], got {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{what} must hold integer link ids, got {t.dtype}")
    t = t.cpu().long()
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= num_links):
        raise ValueError(f"{what} holds a link outside [0, {num_links})")
    return t


def _shapes(in_width, hidden, ch):
    return ((hidden, in_width), (hidden,), (hidden,), (hidden,), (hidden, ch * hidden), (hidden,), (hidden,), (hidden,),
            (1, hidden), (1,))


class SIGNNetTrainer:
    """SIGNNet's ten tensors, both BatchNorms' running statistics and the Adam state on the device.  init = a
    `SIGNNetTwin.state_dict()` (or this class's own) replaces the seeded initial values and reads back bit for bit."""

    def __init__(self, in_width, hidden=256, k_heuristic=0, k_pool_strategy="", dropout=0.5, lr=1e-4, seed=0,
                 device=None, init=None):
        in_width, hidden, dropout, lr = int(in_width), int(hidden), float(dropout), float(lr)
        mode = _pool_mode(k_heuristic, k_pool_strategy)
        _check_shape(hidden, in_width)
        if not 0 <= dropout < 1:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        if not lr > 0 or not np.isfinite(lr):
            raise ValueError(f"lr must be positive and finite, got {lr}")
        self.in_width, self.hidden, self.k_heuristic, self.k_pool_strategy = in_width, hidden, k_heuristic, k_pool_strategy
        self.channels = 1 if mode == 0 else 2
        self.dropout, self.lr, self.seed = dropout, lr, int(seed)
        if init is not None:
            init = self._checked_state(init)
        if device is not None and torch.device(device).type == "cpu":
            raise RuntimeError("SIGNNet training needs a HIP device (MI355X); there is no CPU fallback")
        from .engine import default_engine

        self.engine = default_engine(device)
        self.epochs_done = 0
        self._last_ptr = None
        cfg = N.SignnetCfg(in_width, hidden, mode, self.seed & 0xffffffff, dropout)
        h = C.c_void_p()
        N.check(N.lib().s3grl_signnet_create(self.engine._ctx, C.byref(cfg), C.byref(h)), "s3grl_signnet_create")
        self._h = h
        self.engine._children.add(self)   # the engine closes it before its context goes
        if init is not None:
            self._write(init)

    # -- inputs -----------------------------------------------------------------------------------------------
    def _store(self, rows, row_ptr, y=None):
        """(rows [ΣR, in_width] fp32, row_ptr int64 [L + 1], y fp32 [L] or None) on the engine's device, rows as given
        when they already are (no copy)."""
        dev = self.engine.device
        if rows.dim() < 2 or int(np.prod(rows.shape[1:])) != self.in_width:
            raise ValueError(f"rows must be [ΣR, ...] with {self.in_width} floats per row, got {tuple(rows.shape)}")
        rows = rows.to(device=dev, dtype=torch.float32).contiguous()
        row_ptr = torch.as_tensor(row_ptr)
        if row_ptr.dim() != 1 or row_ptr.numel() < 1 or row_ptr.dtype.is_floating_point:
            raise ValueError("row_ptr must be an integer tensor [L + 1]")
        row_ptr = row_ptr.to(device=dev, dtype=torch.int64).contiguous()
        if y is not None:
            y = torch.as_tensor(y)
            if y.dim() != 1 or y.numel() != row_ptr.numel() - 1:
                raise ValueError(f"y must be [{row_ptr.numel() - 1}], got {tuple(y.shape)}")
            y = y.to(device=dev, dtype=torch.float32).contiguous()
        self._last_ptr = row_ptr
        return rows, row_ptr, y

    # -- training ---------------------------------------------------------------------------------------------
    def fit_epoch(self, rows, row_ptr, y, batch_size=32):
        """One pass over a permutation of the L links in batches of batch_size (a last batch of one link is skipped, as
        `harness.train_and_evaluate` does); returns the per-step losses, fp32 [steps] on the host.  The losses stay on
        the device until the end: one wait per epoch."""
        self._alive()
        batch_size = int(batch_size)
        _check_shape(self.hidden, self.in_width, batch_size)
        rows, row_ptr, y = self._store(rows, row_ptr, y)
        return self._epoch(rows, row_ptr, y, batch_size).cpu()

    def _epoch(self, rows, row_ptr, y, batch_size):
        """fit_epoch on tensors `_store` already checked and moved; the losses stay on the device."""
        L = y.numel()
        if L < 2:
            raise ValueError(f"need two links or more, got {L}")
        steps = -(-(L - 1) // batch_size)
        losses = torch.empty(steps, dtype=torch.float32, device=self.engine.device)
        N.check(N.lib().s3grl_signnet_fit_epoch(self._h, self.epochs_done, N.ptr(rows), rows.shape[0], N.ptr(row_ptr),
                                                N.ptr(y), L, batch_size, self.lr, N.ptr(losses)),
                "s3grl_signnet_fit_epoch")
        self.epochs_done += 1
        return losses

    def draws(self, epoch, step, L, B, row_ptr=None):
        """What the engine draws at (epoch, step) of a pass over L links in batches of B: (link_ids int64 [b], mask1
        uint8 [ΣR_b, hidden], mask2 uint8 [b, hidden]) on the device, b = min(B, L - step · B).  mask1 has one row per
        row of the batch, in batch order, so it needs the store's row_ptr: the one given, or the one of the last
        fit_epoch / step / score call."""
        self._alive()
        epoch, step, L, B = int(epoch), int(step), int(L), int(B)
        _check_shape(self.hidden, self.in_width, B)
        if epoch < 0 or step < 0 or L < 2 or step * B >= L - 1:
            raise ValueError(f"no step {step} of batch size {B} over {L} links")
        ptr = self._last_ptr if row_ptr is None else torch.as_tensor(row_ptr)
        if ptr is None:
            raise ValueError("draws needs row_ptr (none given and no earlier call has seen one)")
        if ptr.numel() != L + 1:
            raise ValueError(f"row_ptr must be [{L + 1}], got {tuple(ptr.shape)}")
        dev, H = self.engine.device, self.hidden
        b = min(B, L - step * B)
        ids = torch.empty(b, dtype=torch.int32, device=dev)
        mask2 = torch.empty((b, H), dtype=torch.uint8, device=dev)
        null = C.c_void_p(0)
        N.check(N.lib().s3grl_signnet_draws(self._h, epoch, step, L, B, N.ptr(ids), null, 0, N.ptr(mask2)),
                "s3grl_signnet_draws")
        ids = ids.long()
        ptr = ptr.to(dev)
        R = int((ptr[ids + 1] - ptr[ids]).sum())
        mask1 = torch.empty((R, H), dtype=torch.uint8, device=dev)
        N.check(N.lib().s3grl_signnet_draws(self._h, epoch, step, L, B, null, N.ptr(mask1), R, null),
                "s3grl_signnet_draws")
        return ids, mask1, mask2

    def step(self, rows, row_ptr, y, link_ids, mask1=None, mask2=None):
        """One Adam step on the links link_ids [B] of the store; mask1 uint8 [ΣR_b, hidden] and mask2 uint8 [B, hidden]
        (non-zero: kept; mask1's rows in batch order) or None for the engine's own draw.  Returns the step's loss."""
        self._alive()
        rows, row_ptr, y = self._store(rows, row_ptr, y)
        L = y.numel()
        ids = _link_ids(link_ids, L)
        B = ids.numel()
        _check_shape(self.hidden, self.in_width, B)
        dev, H = self.engine.device, self.hidden
        ids = ids.to(dev)
        R = int((row_ptr[ids + 1] - row_ptr[ids]).sum())

        def mask(m, n, name):
            if m is None:
                return None
            m = torch.as_tensor(m)
            if tuple(m.shape) != (n, H):
                raise ValueError(f"{name} must be [{n}, {H}], got {tuple(m.shape)}")
            return (m != 0).to(device=dev, dtype=torch.uint8).contiguous()

        mask1, mask2 = mask(mask1, R, "mask1"), mask(mask2, B, "mask2")
        ids32 = ids.to(torch.int32).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        N.check(N.lib().s3grl_signnet_step(self._h, N.ptr(rows), rows.shape[0], N.ptr(row_ptr), N.ptr(y), L,
                                           N.ptr(ids32), B, N.ptr(mask1), N.ptr(mask2), self.lr, N.ptr(loss)),
                "s3grl_signnet_step")
        return float(loss.item())

    def score(self, rows, row_ptr):
        """The logit of every link of the store in eval mode (running statistics, no dropout): fp32 [L] on the device."""
        self._alive()
        rows, row_ptr, _ = self._store(rows, row_ptr)
        L = row_ptr.numel() - 1
        out = torch.empty(L, dtype=torch.float32, device=self.engine.device)
        N.check(N.lib().s3grl_signnet_score(self._h, N.ptr(rows), rows.shape[0], N.ptr(row_ptr), L, N.ptr(out)),
                "s3grl_signnet_score")
        return out

    # -- state ------------------------------------------------------------------------------------------------
    def _read(self, which, shapes):
        n = sum(int(np.prod(s)) for s in shapes)
        flat = torch.empty(n, dtype=torch.float32, device=self.engine.device)
        counters = (C.c_int64 * 3)()
        N.check(N.lib().s3grl_signnet_read_state(self._h, which, N.ptr(flat), counters), "s3grl_signnet_read_state")
        out, o = [], 0
        for s in shapes:
            k = int(np.prod(s))
            out.append(flat[o:o + k].view(s))
            o += k
        return out, [int(c) for c in counters]

    def state_dict(self, optimizer=False):
        """`SIGNNetTwin.state_dict()`'s keys and shapes (device copies): the ten tensors, both BatchNorms' running_mean,
        running_var and num_batches_tracked.  optimizer=True adds "exp_avg." + key and "exp_avg_sq." + key for each of
        the ten and "step", Adam's step count."""
        self._alive()
        shapes = _shapes(self.in_width, self.hidden, self.channels)
        params, counters = self._read(0, shapes)
        out = dict(zip(PARAM_KEYS, params))
        stats, _ = self._read(3, ((self.hidden,),) * 4)
        out.update(zip(STAT_KEYS, stats))
        for key, n in zip(COUNT_KEYS, counters[1:]):
            out[key] = torch.tensor(n, dtype=torch.int64, device=self.engine.device)
        out = {k: out[k] for k in STATE_ORDER}
        if optimizer:
            for name, which in (("exp_avg.", 1), ("exp_avg_sq.", 2)):
                out.update((name + k, t) for k, t in zip(PARAM_KEYS, self._read(which, shapes)[0]))
            out["step"] = counters[0]
        return out

    def _checked_state(self, sd):
        shapes = dict(zip(PARAM_KEYS, _shapes(self.in_width, self.hidden, self.channels)))
        shapes.update((k, (self.hidden,)) for k in STAT_KEYS)
        sd = dict(sd)
        for k, s in shapes.items():
            if k not in sd:
                raise ValueError(f"state_dict lacks {k!r}")
            if tuple(sd[k].shape) != s:
                raise ValueError(f"state_dict[{k!r}] must be {list(s)}, got {list(sd[k].shape)}")
        return sd

    def _write(self, sd):
        dev = self.engine.device

        def flat(keys):
            return torch.cat([torch.as_tensor(sd[k]).to(device=dev, dtype=torch.float32).reshape(-1)
                              for k in keys]).contiguous()

        _, counters = self._read(3, ((self.hidden,),) * 4)
        counters[0] = int(sd.get("step", 0))
        for i, k in enumerate(COUNT_KEYS):
            counters[1 + i] = int(sd.get(k, 0))
        lib = N.lib()
        N.check(lib.s3grl_signnet_write_state(self._h, 0, N.ptr(flat(PARAM_KEYS)), (C.c_int64 * 3)(*counters)),
                "s3grl_signnet_write_state")
        N.check(lib.s3grl_signnet_write_state(self._h, 3, N.ptr(flat(STAT_KEYS)), None), "s3grl_signnet_write_state")
        for name, which in (("exp_avg.", 1), ("exp_avg_sq.", 2)):
            keys = [name + k for k in PARAM_KEYS]
            if all(k in sd for k in keys):
                for k, s in zip(keys, _shapes(self.in_width, self.hidden, self.channels)):
                    if tuple(sd[k].shape) != s:
                        raise ValueError(f"state_dict[{k!r}] must be {list(s)}, got {list(sd[k].shape)}")
                N.check(lib.s3grl_signnet_write_state(self._h, which, N.ptr(flat(keys)), None),
                        "s3grl_signnet_write_state")

    def load_state_dict(self, sd):
        """Takes `SIGNNetTwin.state_dict()` or this class's `state_dict(optimizer=True)`; without the moments Adam's
        stay as they are, without "step" its count restarts at 0."""
        self._alive()
        self._write(self._checked_state(sd))

    def _alive(self):
        if getattr(self, "_h", None) is None:
            raise RuntimeError("SIGNNetTrainer is closed")

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and self.engine._ctx:   # the trainer works on the context's stream
            N.lib().s3grl_signnet_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass



def _per_run(value, n, name):
    """A scalar or a sequence of n -> list of n floats."""
    if isinstance(value, (int, float, np.integer, np.floating)):
        return [float(value)] * n
    out = [float(v) for v in value]
    if len(out) != n:
        raise ValueError(f"{name} must be a scalar or one value per seed ({n}), got {len(out)}")
    return out


class SIGNNetRuns:
    """The runs of one config, trained side by side: `.members[r]` is an ordinary `SIGNNetTrainer` of seeds[r], and a
    group epoch leaves each of them bit-identical to what its own `fit_epoch` computes (s3grl_signnetruns_fit_epoch:
    the step kernels with a second grid dimension, the run; four launches per step for all of them).  The members stay
    usable alone, but a group epoch needs every member at the group's epoch."""

    def __init__(self, in_width, hidden=256, k_heuristic=0, k_pool_strategy="", dropout=0.5, lr=1e-4, seeds=(0,),
                 device=None):
        seeds = [int(s) for s in seeds]
        if not seeds:
            raise ValueError("seeds must name one run or more")
        if len(seeds) > N.SIGNNET_MAX_RUNS:
            raise NotImplementedError(f"SIGNNet runs above {N.SIGNNET_MAX_RUNS} in one group, got {len(seeds)}")
        dropout, lr = _per_run(dropout, len(seeds), "dropout"), _per_run(lr, len(seeds), "lr")
        self.seeds, self.epochs_done, self.members = tuple(seeds), 0, []
        try:
            for seed, p, rate in zip(seeds, dropout, lr):
                self.members.append(SIGNNetTrainer(in_width, hidden, k_heuristic, k_pool_strategy, p, rate, seed=seed,
                                                   device=device))
        except Exception:
            self.close()
            raise
        self.engine = self.members[0].engine

    def _alive(self):
        for m in self.members:
            m._alive()
            if m.epochs_done != self.epochs_done:
                raise ValueError(f"the member of seed {m.seed} is at epoch {m.epochs_done}, the group at "
                                 f"{self.epochs_done}: a group epoch needs every member at the group's epoch")

    def fit_epoch(self, rows, row_ptr, y, batch_size=32):
        """`SIGNNetTrainer.fit_epoch` for every member at once; returns the per-step losses, fp32 [R, steps] on the
        host.  One wait per epoch."""
        self._alive()
        batch_size = int(batch_size)
        lead = self.members[0]
        _check_shape(lead.hidden, lead.in_width, batch_size)
        rows, row_ptr, y = lead._store(rows, row_ptr, y)
        return self._epoch(rows, row_ptr, y, batch_size).cpu()

    def _epoch(self, rows, row_ptr, y, batch_size):
        """fit_epoch on tensors `_store` already checked and moved; the losses stay on the device."""
        self._alive()
        L, R = y.numel(), len(self.members)
        if L < 2:
            raise ValueError(f"need two links or more, got {L}")
        steps = -(-(L - 1) // batch_size)
        losses = torch.empty((R, steps), dtype=torch.float32, device=self.engine.device)
        handles = (C.c_void_p * R)(*[m._h.value for m in self.members])
        lr = (C.c_double * R)(*[m.lr for m in self.members])
        N.check(N.lib().s3grl_signnetruns_fit_epoch(handles, R, self.epochs_done, N.ptr(rows), rows.shape[0],
                                                      N.ptr(row_ptr), N.ptr(y), L, batch_size, lr, N.ptr(losses)),
                "s3grl_signnetruns_fit_epoch")
        self.epochs_done += 1
        for m in self.members:
            m.epochs_done += 1
            m._last_ptr = row_ptr
        return losses

    def score(self, rows, row_ptr):
        """Every member's eval-mode logits of every link of the store: fp32 [R, L] on the device."""
        for m in self.members:
            m._alive()
        return torch.stack([m.score(rows, row_ptr) for m in self.members])

    def state_dict(self, optimizer=False):
        """[`SIGNNetTrainer.state_dict(optimizer)` of each member]"""
        return [m.state_dict(optimizer) for m in self.members]

    def load_state_dict(self, sds):
        """One state dict per member, as `SIGNNetTrainer.load_state_dict` takes them."""
        sds = list(sds)
        if len(sds) != len(self.members):
            raise ValueError(f"need one state dict per member ({len(self.members)}), got {len(sds)}")
        for m, sd in zip(self.members, sds):
            m.load_state_dict(sd)

    def close(self):
        for m in self.members:
            m.close()
