"""Test infrastructure: a pure-torch restatement (fp64 by default, any device) of raw-edge message passing and of the
models built on it, written from the definitions (PyG 2.0.x SAGEConv, GINConv, global_mean_pool; reference
models.py:78-135 SAGE, :225-298 GIN; baselines/gnn_link_pred.py Net).  It checks s3grl_amd.mpnn / mpgnn; the product
never imports it.

    out = aggregate_sum(h, src, dst)            # out[i] = Σ_{j -> i} h[j], every listed arc once, loops included
    out = aggregate_mean(h, src, dst)           # ... / max(indeg(i), 1)
    g_h = aggregate_mean_t(g_out, src, dst)     # the transposed operators: what the backward computes
    logits = sage_forward(state_dict, z, x, edge_index, node_ptr, num_convs=3)

The models take their parameters from a state_dict (the twin's).  training=False: BatchNorm with its running
statistics; training=True: with the batch's own (biased variance), dropout taken as 0.
"""
import torch

from seal_nn_reference import gcn_norm, node_input, propagate


def _arcs(src, dst):
    return torch.as_tensor(src).long(), torch.as_tensor(dst).long()


def in_degree(dst, n):
    dst = torch.as_tensor(dst).long()
    return torch.zeros(n, dtype=torch.float64, device=dst.device).index_add_(0, dst, torch.ones_like(dst,
                                                                                                      dtype=torch.float64))


def aggregate_sum(h, src, dst):
    src, dst = _arcs(src, dst)
    out = torch.zeros_like(h)
    chunk = max((1 << 26) // max(h.shape[1], 1), 1)           # arcs taken so that a gathered block stays small
    for a in range(0, src.numel(), chunk):
        out = out.index_add(0, dst[a:a + chunk], h[src[a:a + chunk]])
    return out


def aggregate_mean(h, src, dst):
    cnt = in_degree(dst, h.shape[0]).clamp(min=1).to(h.dtype)
    return aggregate_sum(h, src, dst) / cnt[:, None]


def aggregate_sum_t(g, src, dst):
    """Transpose of aggregate_sum: gh[j] = Σ_{j -> i} g[i]."""
    return aggregate_sum(g, dst, src)


def aggregate_mean_t(g, src, dst):
    """Transpose of aggregate_mean: gh[j] = Σ_{j -> i} g[i] / max(indeg(i), 1): the DESTINATION's degree."""
    cnt = in_degree(dst, g.shape[0]).clamp(min=1).to(g.dtype)
    return aggregate_sum(g / cnt[:, None], dst, src)


def aggregate_mean_t_wrong_side(g, src, dst):
    """What a backward that scaled by its OWN row's degree would give (a graph must tell this from the above)."""
    cnt = in_degree(dst, g.shape[0]).clamp(min=1).to(g.dtype)
    return aggregate_sum(g, dst, src) / cnt[:, None]


def segment_mean(x, node_ptr):
    """out[g] = Σ rows / max(n_g, 1); a zero row for an empty graph."""
    node_ptr = torch.as_tensor(node_ptr).long().to(x.device)
    counts = node_ptr.diff()
    G = counts.numel()
    graph = torch.repeat_interleave(torch.arange(G, device=x.device), counts, output_size=x.shape[0])
    out = torch.zeros((G, x.shape[1]), dtype=x.dtype, device=x.device).index_add(0, graph, x)
    return out / counts.clamp(min=1).to(x.dtype)[:, None]


def _p(sd, key, like):
    return sd[key].to(dtype=like.dtype, device=like.device)


def _linear(sd, prefix, x, bias=True):
    out = x @ _p(sd, prefix + ".weight", x).T
    return out + _p(sd, prefix + ".bias", x) if bias else out


def _bn(sd, prefix, x, training, eps=1e-5):
    if training:
        mean, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mean, var = _p(sd, prefix + ".running_mean", x), _p(sd, prefix + ".running_var", x)
    return (x - mean) / torch.sqrt(var + eps) * _p(sd, prefix + ".weight", x) + _p(sd, prefix + ".bias", x)


def _mlp(sd, prefix, x, training):
    i = 0
    while f"{prefix}.lins.{i + 1}.weight" in sd:
        x = torch.relu(_bn(sd, f"{prefix}.norms.{i}", _linear(sd, f"{prefix}.lins.{i}", x), training))
        i += 1
    return _linear(sd, f"{prefix}.lins.{i}", x)


def _input(sd, z, x, dtype):
    h = node_input(sd, z, x)                      # fp64
    return h.to(dtype)


def sage_conv(sd, prefix, x, src, dst):
    return _linear(sd, prefix + ".lin_l", aggregate_mean(x, src, dst)) + _linear(sd, prefix + ".lin_r", x, bias=False)


def gin_conv(sd, prefix, x, src, dst, training, batch_norm=True):
    h = (1 + _p(sd, prefix + ".eps", x)) * x + aggregate_sum(x, src, dst)
    h = torch.relu(_linear(sd, prefix + ".nn.0", h))
    h = torch.relu(_linear(sd, prefix + ".nn.2", h))
    return _bn(sd, prefix + ".nn.4", h, training) if batch_norm else h


def sage_forward(sd, z, x, edge_index, node_ptr, *, num_convs, training=False, dtype=torch.float64):
    """Reference SAGE (dropout 0): logits [G, 1]."""
    src, dst = _arcs(edge_index[0], edge_index[1])
    h = _input(sd, z, x, dtype)
    for i in range(num_convs):
        h = sage_conv(sd, f"convs.{i}", h, src, dst)
        if i < num_convs - 1:
            h = torch.relu(h)
    first = torch.as_tensor([int(v) for v in node_ptr[:-1]], device=h.device)
    return _mlp(sd, "mlp", h[first] * h[first + 1], training)


def gin_forward(sd, z, x, edge_index, node_ptr, *, num_layers, jk=True, training=False, dtype=torch.float64):
    """Reference GIN (dropout 0): logits [G, 1]."""
    src, dst = _arcs(edge_index[0], edge_index[1])
    h = gin_conv(sd, "conv1", _input(sd, z, x, dtype), src, dst, training)
    hs = [h]
    for i in range(num_layers - 1):
        h = gin_conv(sd, f"convs.{i}", h, src, dst, training)
        hs.append(h)
    h = torch.cat(hs, 1) if jk else hs[-1]
    return _mlp(sd, "mlp", segment_mean(h, node_ptr), training)


def net_forward(sd, x, edge_index, num_nodes, layer, dtype=torch.float64):
    """gnn_link_pred.Net.encode without dropout: z [N, hidden].  x = None is eye(N)."""
    src, dst = _arcs(edge_index[0], edge_index[1])
    h = torch.eye(num_nodes, dtype=dtype, device=src.device) if x is None else x.to(dtype)
    if layer == "GCN":
        gs, gd, coef = gcn_norm(edge_index, num_nodes)
    for i in (1, 2, 3):
        p = f"conv{i}"
        if layer == "GCN":
            h = propagate(h @ _p(sd, p + ".lin.weight", h).T, gs, gd, coef.to(dtype)) + _p(sd, p + ".bias", h)
        elif layer == "SAGE":
            h = sage_conv(sd, p, h, src, dst)
        elif layer == "GIN":
            h = gin_conv(sd, p, h, src, dst, False, batch_norm=False)
        else:
            raise NotImplementedError(layer)
        if i < 3:
            h = torch.relu(h)
    return h


class torch_operators:
    """Context manager: s3grl_amd.mpnn's two graph operators replaced by their torch restatement in the input's own
    precision (index_add over op.edge_index, scatter-style mean pool), so that a twin trains by the same loop
    without the HIP kernels.  This is how the end-to-end AUC thresholds were measured."""

    def __enter__(self):
        from s3grl_amd import mpnn

        self.mpnn, self.saved = mpnn, (mpnn.aggregate, mpnn.segment_mean)

        def aggregate(h, op, mode, self_coef=0.0):
            ei = op.edge_index
            out = (aggregate_mean if mode == "mean" else aggregate_sum)(h, ei[0], ei[1])
            return out + self_coef * h if self_coef else out

        mpnn.aggregate = aggregate
        mpnn.segment_mean = lambda x, node_ptr, max_nodes=None: segment_mean(x, node_ptr)
        return self

    def __exit__(self, *exc):
        self.mpnn.aggregate, self.mpnn.segment_mean = self.saved
        return False
