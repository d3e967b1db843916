"""The MF row of the reference's Table 2 (baselines/mf.py train_mf, run_helpers/run_mf.py): a learnable
`nn.Embedding(N, hidden)` and a `LinkPredictor` MLP over the Hadamard product of the two endpoint rows, trained by
dense `torch.optim.Adam` in batches of positive links and as many uniform random pairs, whose every step runs as two
HIP kernels behind the C ABI (s3grl_mf_*, csrc/s3grl_mf.hip).

    auc = train_mf(data, split_edge, device, 1, 3, 32, 0.5, 32, 0.01, 50, 1, 1, seed, args)    # the reference's call
    results = run_mf(split)                                        # {'AUC': (val, test), 'AP': (val, test)}
    mf = MFTrainer(N, 32, 3, 0.5, 0.01, seed=1); loss = mf.fit_epoch(pos_train, 32); s = mf.score(pairs)

Same algorithm as the reference: per epoch a permutation of the train links in batches (the last one short); per batch
`randint(0, N)` negative pairs (self-pairs and true edges allowed), two predictor evaluations with independent dropout
masks, `-log(s + 1e-15).mean()` / `-log(1 - s + 1e-15).mean()` with the sigmoid in fp32, and one dense Adam step over
the whole table and the predictor: a row no pair touches still decays its moments and still moves once they are
non-zero.  The table starts as N(0, 1), every Linear layer uniform in ±1/sqrt(fan_in).  All draws (initial values,
permutations, negatives, dropout masks) come from the engine's counter-based generator keyed by (seed, epoch, step,
index), not from torch's streams, so results are NOT bit-equal to the reference's: same algorithm, same distributions,
same update given the same pairs and masks.  Two runs with one seed are bit-identical.  GPU only; no CPU fallback.
Shapes no reference run uses raise NotImplementedError: hidden > 128, num_layers outside 2..4, batch_size > 1024.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _native as N


def _check_shape(hidden, num_layers, batch_size=1):
    if hidden < 1 or batch_size < 1:
        raise ValueError(f"need hidden >= 1 and batch_size >= 1, got {hidden} and {batch_size}")
    if hidden > N.MF_MAX_HIDDEN:
        raise NotImplementedError(f"MF with hidden_channels above {N.MF_MAX_HIDDEN}, got {hidden}")
    if not N.MF_MIN_LAYERS <= num_layers <= N.MF_MAX_LAYERS:
        raise NotImplementedError(f"MF with num_layers outside {N.MF_MIN_LAYERS}..{N.MF_MAX_LAYERS}, got {num_layers}")
    if batch_size > N.MF_MAX_BATCH:
        raise NotImplementedError(f"MF with batch_size above {N.MF_MAX_BATCH}, got {batch_size}")


def layout(hidden, num_layers, batch):
    """The lane layout of the step kernels, without a GPU: dict(channels_per_lane, lanes_per_pair, pairs_per_tile,
    tiles).  A pair (and a table row of the update) is worked on by lanes_per_pair lanes, each channels_per_lane
    channels; a workgroup takes pairs_per_tile of the step's 2·batch pairs."""
    hidden, num_layers, batch = int(hidden), int(num_layers), int(batch)
    _check_shape(hidden, num_layers, batch)
    out = (C.c_int32 * 4)()
    N.check(N.lib().s3grl_mf_layout(hidden, num_layers, batch, out), "s3grl_mf_layout")
    return {"channels_per_lane": out[0], "lanes_per_pair": out[1], "pairs_per_tile": out[2], "tiles": out[3]}


def num_predictor_params(hidden, num_layers):
    return (num_layers - 1) * (hidden * hidden + hidden) + hidden + 1


def _pairs(p, num_nodes, what, empty_ok=False):
    """[P, 2] integer node ids in [0, num_nodes) -> int64 CPU tensor."""
    t = p if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p))
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"{what} must be [P, 2], got {tuple(t.shape)}")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"{what} must hold integer node ids, got {t.dtype}")
    if not empty_ok and not t.shape[0]:
        raise ValueError(f"{what} is empty")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= num_nodes):
        raise ValueError(f"{what} holds a node outside [0, {num_nodes})")
    return t


class MFTrainer:
    """The embedding table, the predictor and their Adam state on the device.  init = (table [N, hidden], [(weight
    [out, hidden], bias [out]) per layer]) replaces the seeded initial values and is read back bit for bit."""

    def __init__(self, num_nodes, hidden, num_layers, dropout, lr, seed=0, device=None, init=None):
        num_nodes, hidden, num_layers = int(num_nodes), int(hidden), int(num_layers)
        dropout, lr = float(dropout), float(lr)
        if num_nodes < 1 or num_nodes >= 1 << 31:
            raise ValueError(f"num_nodes must be in [1, 2^31), got {num_nodes}")
        _check_shape(hidden, num_layers)
        if not 0 <= dropout < 1:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        if not lr > 0 or not np.isfinite(lr):
            raise ValueError(f"lr must be positive and finite, got {lr}")
        self.num_nodes, self.hidden, self.num_layers = num_nodes, hidden, num_layers
        self.dropout, self.lr, self.seed = dropout, lr, int(seed)
        table0 = pred0 = None
        if init is not None:
            table0, layers0 = init
            table0 = torch.as_tensor(table0, dtype=torch.float32)
            if tuple(table0.shape) != (num_nodes, hidden):
                raise ValueError(f"init table must be [{num_nodes}, {hidden}], got {tuple(table0.shape)}")
            if len(layers0) != num_layers:
                raise ValueError(f"init needs {num_layers} (weight, bias) pairs, got {len(layers0)}")
            flat = []
            for l, (w, b) in enumerate(layers0):
                out = 1 if l == num_layers - 1 else hidden
                w, b = torch.as_tensor(w, dtype=torch.float32), torch.as_tensor(b, dtype=torch.float32)
                if tuple(w.shape) != (out, hidden) or tuple(b.shape) != (out,):
                    raise ValueError(f"init layer {l} must be ([{out}, {hidden}], [{out}]), got "
                                     f"({tuple(w.shape)}, {tuple(b.shape)})")
                flat += [w.reshape(-1).cpu(), b.reshape(-1).cpu()]
            pred0 = torch.cat(flat)
        if device is not None and torch.device(device).type == "cpu":
            raise RuntimeError("MF training needs a HIP device (MI355X); there is no CPU fallback")
        from .engine import default_engine

        self.engine = default_engine(device)
        dev = self.engine.device
        self.epochs_done = 0
        cfg = N.MfCfg(hidden, num_layers, dropout, self.seed & 0xffffffff)
        t0 = None if table0 is None else table0.to(dev).contiguous()
        p0 = None if pred0 is None else pred0.to(dev).contiguous()
        h = C.c_void_p()
        N.check(N.lib().s3grl_mf_create(self.engine._ctx, num_nodes, C.byref(cfg), N.ptr(t0), N.ptr(p0), C.byref(h)),
                "s3grl_mf_create")
        self._h = h
        self.engine._children.add(self)   # the engine closes it before its context goes

    # -- training ---------------------------------------------------------------------------------------------
    def _train_list(self, pos_train):
        t = _pairs(pos_train, self.num_nodes, "pos_train")
        return t.to(device=self.engine.device, dtype=torch.int32).contiguous()

    def fit_epoch(self, pos_train, batch_size):
        """One pass over a permutation of pos_train [E, 2] in batches of batch_size; returns the epoch's loss,
        Σ loss·B over Σ B.  The step losses stay on the device until the end: no sync per step."""
        self._alive()
        _check_shape(self.hidden, self.num_layers, int(batch_size))
        return self._epoch(self._train_list(pos_train), int(batch_size))

    def _epoch(self, train, batch_size):
        """fit_epoch on a list that `_train_list` already checked and moved."""
        E = train.shape[0]
        steps = -(-E // batch_size)
        losses = torch.empty(steps, dtype=torch.float32, device=self.engine.device)
        N.check(N.lib().s3grl_mf_epoch(self._h, self.epochs_done, N.ptr(train), E, batch_size, self.lr,
                                       N.ptr(losses)), "s3grl_mf_epoch")
        self.epochs_done += 1
        sizes = np.full(steps, batch_size, dtype=np.float64)
        sizes[-1] = E - (steps - 1) * batch_size
        return float((losses.cpu().double().numpy() * sizes).sum() / E)

    def draws(self, epoch, step, num_train, batch_size):
        """What the engine draws at (epoch, step) of a pass over num_train links: (pos_idx int64 [B] positions in the
        train list, neg int64 [B, 2], masks uint8 [2B, num_layers - 1, hidden], positives first), on the device."""
        self._alive()
        epoch, step, num_train, batch_size = int(epoch), int(step), int(num_train), int(batch_size)
        _check_shape(self.hidden, self.num_layers, batch_size)
        B = min(batch_size, num_train - step * batch_size)
        if B < 1 or epoch < 0 or step < 0:
            raise ValueError(f"no step {step} of batch size {batch_size} over {num_train} links")
        dev = self.engine.device
        idx = torch.empty(B, dtype=torch.int32, device=dev)
        neg = torch.empty((B, 2), dtype=torch.int32, device=dev)
        masks = torch.empty((2 * B, self.num_layers - 1, self.hidden), dtype=torch.uint8, device=dev)
        N.check(N.lib().s3grl_mf_export_draws(self._h, epoch, step, num_train, batch_size, N.ptr(idx), N.ptr(neg),
                                              N.ptr(masks)), "s3grl_mf_export_draws")
        return idx.long(), neg.long(), masks

    def step(self, pos_pairs, neg_pairs, masks=None):
        """One Adam step on the given pairs ([B, 2] each); masks uint8 [2B, num_layers - 1, hidden] (non-zero: kept;
        positives first) or None for the engine's own draw.  Returns the step's loss."""
        self._alive()
        pos = _pairs(pos_pairs, self.num_nodes, "pos_pairs")
        neg = _pairs(neg_pairs, self.num_nodes, "neg_pairs")
        if pos.shape[0] != neg.shape[0]:
            raise ValueError(f"need as many negative pairs as positive ones, got {neg.shape[0]} and {pos.shape[0]}")
        B = pos.shape[0]
        _check_shape(self.hidden, self.num_layers, B)
        dev = self.engine.device
        pairs = torch.cat([pos.to(dev), neg.to(dev)]).to(torch.int32).contiguous()
        if masks is not None:
            masks = torch.as_tensor(masks)
            if tuple(masks.shape) != (2 * B, self.num_layers - 1, self.hidden):
                raise ValueError(f"masks must be [{2 * B}, {self.num_layers - 1}, {self.hidden}], got "
                                 f"{tuple(masks.shape)}")
            masks = (masks != 0).to(device=dev, dtype=torch.uint8).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        N.check(N.lib().s3grl_mf_step_pairs(self._h, N.ptr(pairs), B, N.ptr(masks), self.lr, N.ptr(loss)),
                "s3grl_mf_step_pairs")
        return float(loss.item())

    def score(self, pairs):
        """sigmoid(predictor(x[a] ⊙ x[b])) in eval mode of pairs [P, 2]: fp32 [P] on the device."""
        self._alive()
        p = _pairs(pairs, self.num_nodes, "pairs", empty_ok=True)
        dev = self.engine.device
        p = p.to(device=dev, dtype=torch.int32).contiguous()
        out = torch.empty(p.shape[0], dtype=torch.float32, device=dev)
        N.check(N.lib().s3grl_mf_score(self._h, N.ptr(p), p.shape[0], N.ptr(out)), "s3grl_mf_score")
        return out

    # -- state ------------------------------------------------------------------------------------------------
    def state(self):
        """dict(weight, exp_avg, exp_avg_sq: fp32 [N, hidden]; layers, layers_exp_avg, layers_exp_avg_sq: a list of
        (weight [out, hidden], bias [out]) per layer; step: Adam's step count), device copies."""
        self._alive()
        dev, H = self.engine.device, self.hidden
        P = num_predictor_params(H, self.num_layers)
        tabs = [torch.empty((self.num_nodes, H), dtype=torch.float32, device=dev) for _ in range(3)]
        flats = [torch.empty(P, dtype=torch.float32, device=dev) for _ in range(3)]
        steps = C.c_int64()
        N.check(N.lib().s3grl_mf_state(self._h, *(N.ptr(t) for t in tabs), *(N.ptr(f) for f in flats),
                                       C.byref(steps)), "s3grl_mf_state")

        def layers(flat):
            out, o = [], 0
            for l in range(self.num_layers):
                rows = 1 if l == self.num_layers - 1 else H
                out.append((flat[o:o + rows * H].view(rows, H), flat[o + rows * H:o + rows * H + rows]))
                o += rows * H + rows
            return out

        return {"weight": tabs[0], "exp_avg": tabs[1], "exp_avg_sq": tabs[2], "layers": layers(flats[0]),
                "layers_exp_avg": layers(flats[1]), "layers_exp_avg_sq": layers(flats[2]), "step": int(steps.value)}

    def _alive(self):
        if getattr(self, "_h", None) is None:
            raise RuntimeError("MFTrainer is closed")

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and self.engine._ctx:   # the trainer works on the context's stream
            N.lib().s3grl_mf_destroy(h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the reference's loop ------------------------------------------------------------------------------------------
def _evaluate(mf, lists):
    from .heuristics import average_precision, roc_auc

    out = {}
    for name, (pos, neg) in lists.items():
        s = mf.score(torch.cat([pos, neg])).cpu().numpy()
        y = np.r_[np.ones(len(pos)), np.zeros(len(neg))]
        out[name] = (roc_auc(y, s), average_precision(y, s))
    return {"AUC": (out["valid"][0], out["test"][0]), "AP": (out["valid"][1], out["test"][1])}


def _train_run(num_nodes, split_edge, *, num_layers, hidden, dropout, batch_size, lr, epochs, eval_steps, seed, device,
               on_eval=None):
    """One run of train_mf's loop: per-eval results {'AUC': [(val, test)], 'AP': [...]}."""
    num_nodes, epochs, eval_steps, batch_size = int(num_nodes), int(epochs), int(eval_steps), int(batch_size)
    if epochs < 0 or eval_steps < 1:
        raise ValueError("need epochs >= 0 and eval_steps >= 1")
    for s in ("train", "valid", "test"):
        if s not in split_edge or "edge" not in split_edge[s] or (s != "train" and "edge_neg" not in split_edge[s]):
            raise ValueError("split_edge needs train / valid / test with 'edge' (and 'edge_neg' for valid and test)")
    train = _pairs(split_edge["train"]["edge"], num_nodes, "split_edge['train']['edge']")
    lists = {s: (_pairs(split_edge[s]["edge"], num_nodes, f"split_edge['{s}']['edge']"),
                 _pairs(split_edge[s]["edge_neg"], num_nodes, f"split_edge['{s}']['edge_neg']"))
             for s in ("valid", "test")}
    _check_shape(int(hidden), int(num_layers), batch_size)
    mf = MFTrainer(num_nodes, hidden, num_layers, dropout, lr, seed=seed, device=device)
    try:
        train_dev = mf._train_list(train)
        results = {"AUC": [], "AP": []}
        for epoch in range(1, epochs + 1):
            loss = mf._epoch(train_dev, batch_size)
            if epoch % eval_steps == 0:
                res = _evaluate(mf, lists)
                for key in results:
                    results[key].append(res[key])
                if on_eval is not None:
                    on_eval(epoch, loss, res)
    finally:
        mf.close()
    return results


def train_mf(data, split_edge, device, log_steps, num_layers, hidden_channels, dropout, batch_size, lr, epochs,
             eval_steps, runs, seed, args):
    """Reference baselines/mf.train_mf: `runs` runs (each re-seeded with `seed` and reset, as the reference does) of
    `epochs` epochs, evaluated every eval_steps epochs on split_edge's valid / test 'edge' and 'edge_neg'.  `data`
    needs `.num_nodes`; split_edge is `workloads.Split.split_edge()`.  Returns the test AUC · 100 at the first
    evaluation of maximal validation AUC of the FIRST run, which is what Logger.print_statistics hands back (every
    run repeats it: one seed, one result).  The reference's log lines go to args.res_dir/log.txt only when args.res_dir is
    set; nothing is printed."""
    from .gae import best_at_first_max

    runs, log_steps = int(runs), int(log_steps)
    if runs < 1 or log_steps < 1:
        raise ValueError("need runs >= 1 and log_steps >= 1")
    res_dir = getattr(args, "res_dir", "") or ""
    log_file = os.path.join(res_dir, "log.txt") if res_dir else None
    finals = []
    for run in range(runs):
        def on_eval(epoch, loss, res, run=run):
            if log_file is not None and epoch % log_steps == 0:
                with open(log_file, "a") as f:
                    for key, (v, t) in res.items():
                        print(f"{key}\nRun: {run + 1:02d}, Epoch: {epoch:02d}, Loss: {loss:.4f}, Valid: {100 * v:.2f}%, "
                              f"Test: {100 * t:.2f}%", file=f)

        results = _train_run(data.num_nodes, split_edge, num_layers=num_layers, hidden=hidden_channels, dropout=dropout,
                             batch_size=batch_size, lr=lr, epochs=epochs, eval_steps=eval_steps, seed=seed,
                             device=device, on_eval=on_eval)
        if not results["AUC"]:
            raise ValueError("no evaluation ran: epochs < eval_steps")
        r = (100 * torch.tensor(results["AUC"])).numpy()   # fp32, as Logger.print_statistics
        finals.append(float(best_at_first_max(r)[1]))
    return finals[0]


def run_mf(split, *, epochs=50, hidden=32, num_layers=3, dropout=0.5, batch_size=32, lr=0.01, seed=1, device=None):
    """One Table 2 MF row from a `workloads.Split` (run_helpers/run_mf.py: 50 epochs, hidden 32, 3 layers, dropout
    0.5, batches of 32, lr 0.01, eval every epoch): {'AUC': (best val, test at it), 'AP': (...)}, each chosen at the
    first epoch of its own maximal val value, as fractions (like run_gae)."""
    from .gae import best_at_first_max

    results = _train_run(split.num_nodes, split.split_edge(), num_layers=num_layers, hidden=hidden, dropout=dropout,
                         batch_size=batch_size, lr=lr, epochs=epochs, eval_steps=1, seed=seed, device=device)
    if not results["AUC"]:
        raise ValueError("epochs must be >= 1")
    return {k: tuple(float(v) for v in best_at_first_max(r)) for k, r in results.items()}
