"""s3grl_amd — MI355X (gfx950) engine for the S3GRL PoS / PoS Plus / SoP operator precompute.

Only the hot path of venomouscyanide/S3GRL lives here: the HIP kernels and
C ABI in csrc/ + include/s3grl.h, and the host-side mirror of the reference's operator
interface (`s3grl_amd.tuned_SIGN`).  Importing the package does not touch the GPU; the first
call into the engine loads libs3grl_hip.so and fails loudly if it is not built.
"""
__version__ = "0.1.0"


def precompute(*args, **kwargs):
    """See `s3grl_amd.engine.precompute` (imported lazily: the engine imports torch)."""
    from .engine import precompute as _p

    return _p(*args, **kwargs)


def extract_enclosing_subgraphs(*args, **kwargs):
    """See `s3grl_amd.dataset.extract_enclosing_subgraphs` (reference utils.py:446-554)."""
    from .dataset import extract_enclosing_subgraphs as _f

    return _f(*args, **kwargs)


def process_split(*args, **kwargs):
    """See `s3grl_amd.dataset.process_split` (reference sgrl_link_pred.py:96-220)."""
    from .dataset import process_split as _f

    return _f(*args, **kwargs)


def enclosing_subgraphs(*args, **kwargs):
    """See `s3grl_amd.seal.enclosing_subgraphs`: the labelled enclosing subgraphs of the SEAL baselines
    (reference utils.py:556-573, k_hop_subgraph + construct_pyg_graph) on the GPU."""
    from .seal import enclosing_subgraphs as _f

    return _f(*args, **kwargs)


def node_2_vec_pretrain(*args, **kwargs):
    """See `s3grl_amd.node2vec.node_2_vec_pretrain` (reference n2v_prep.py): node2vec features on the GPU."""
    from .node2vec import node_2_vec_pretrain as _f

    return _f(*args, **kwargs)


def Node2Vec(*args, **kwargs):
    """See `s3grl_amd.node2vec.Node2Vec`: PyG Node2Vec (p = q = 1, sparse) trained by SparseAdam on the GPU."""
    from .node2vec import Node2Vec as _c

    return _c(*args, **kwargs)


def Heuristics(*args, **kwargs):
    """See `s3grl_amd.heuristics.Heuristics`: CN, AA, PPR, RA, Jaccard, PA and Katz link scores of one
    graph on the GPU."""
    from .heuristics import Heuristics as _c

    return _c(*args, **kwargs)


def run_heuristic(*args, **kwargs):
    """See `s3grl_amd.heuristics.run_heuristic` (reference `--use_heuristic`): a Table 2 heuristic row."""
    from .heuristics import run_heuristic as _f

    return _f(*args, **kwargs)


def SketchGraph(*args, **kwargs):
    """See `s3grl_amd.sketch.SketchGraph`: MinHash / HyperLogLog sketches of every node's k-hop balls and the
    per-link structure features estimated from them (ELPH / BUDDY), on the GPU."""
    from .sketch import SketchGraph as _c

    return _c(*args, **kwargs)


def BuddyTwin(*args, **kwargs):
    """See `s3grl_amd.sketch.BuddyTwin`: BUDDY's predictor over the sketch features and propagated node features."""
    from .sketch import BuddyTwin as _c

    return _c(*args, **kwargs)


def run_buddy(*args, **kwargs):
    """See `s3grl_amd.sketch.run_buddy`: the BUDDY row from a split."""
    from .sketch import run_buddy as _f

    return _f(*args, **kwargs)


def CommonNeighbours(*args, **kwargs):
    """See `s3grl_amd.ncn.CommonNeighbours`: every link's common-neighbour list and its transpose, on the GPU.  (The
    name `s3grl_amd.ncn` is the module.)"""
    from .ncn import CommonNeighbours as _c

    return _c(*args, **kwargs)


def common_neighbour_sum(*args, **kwargs):
    """See `s3grl_amd.ncn.common_neighbour_sum`: C[l] = Σ z[w] over a link's common neighbours, differentiable in z."""
    from .ncn import common_neighbour_sum as _f

    return _f(*args, **kwargs)


def NCNTwin(*args, **kwargs):
    """See `s3grl_amd.ncn.NCNTwin`: Neural Common Neighbour's predictor on a whole-graph GCN encoder."""
    from .ncn import NCNTwin as _c

    return _c(*args, **kwargs)


def run_ncn(*args, **kwargs):
    """See `s3grl_amd.ncn.run_ncn`: the NCN row from a split."""
    from .ncn import run_ncn as _f

    return _f(*args, **kwargs)


def SplitNeighbours(*args, **kwargs):
    """See `s3grl_amd.ncn.SplitNeighbours`: per link the common neighbours and each endpoint's own, on the GPU."""
    from .ncn import SplitNeighbours as _c

    return _c(*args, **kwargs)


def completed_neighbour_sum(*args, **kwargs):
    """See `s3grl_amd.ncn.completed_neighbour_sum`: C[l] = Σ weight·z[w] over a link's split list, differentiable in z
    and in the weights."""
    from .ncn import completed_neighbour_sum as _f

    return _f(*args, **kwargs)


def NCNCTwin(*args, **kwargs):
    """See `s3grl_amd.ncn.NCNCTwin`: NCN with its common-neighbour pool completed (NCNC)."""
    from .ncn import NCNCTwin as _c

    return _c(*args, **kwargs)


def run_ncnc(*args, **kwargs):
    """See `s3grl_amd.ncn.run_ncnc`: the NCNC row from a split."""
    from .ncn import run_ncnc as _f

    return _f(*args, **kwargs)


def run_vgae(*args, **kwargs):
    """See `s3grl_amd.gae.run_vgae` (reference baselines/vgae.run_vgae): GAE / VGAE / ARGVA on the GPU."""
    from .gae import run_vgae as _f

    return _f(*args, **kwargs)


def run_gae(*args, **kwargs):
    """See `s3grl_amd.gae.run_gae`: a Table 2 autoencoder row (GAE, VGAE or ARGVA) from a split."""
    from .gae import run_gae as _f

    return _f(*args, **kwargs)


def train_mf(*args, **kwargs):
    """See `s3grl_amd.mf.train_mf` (reference baselines/mf.train_mf): the MF baseline on the GPU."""
    from .mf import train_mf as _f

    return _f(*args, **kwargs)


def run_mf(*args, **kwargs):
    """See `s3grl_amd.mf.run_mf`: the Table 2 MF row from a split."""
    from .mf import run_mf as _f

    return _f(*args, **kwargs)


def MFTrainer(*args, **kwargs):
    """See `s3grl_amd.mf.MFTrainer`: the embedding table, the predictor and their dense Adam state on the GPU."""
    from .mf import MFTrainer as _c

    return _c(*args, **kwargs)


def SIGNNetTrainer(*args, **kwargs):
    """See `s3grl_amd.signnet.SIGNNetTrainer`: SIGNNet trained on the engine's rows by fused HIP step kernels."""
    from .signnet import SIGNNetTrainer as _c

    return _c(*args, **kwargs)


def SIGNNetRuns(*args, **kwargs):
    """See `s3grl_amd.signnet.SIGNNetRuns`: the runs of a config trained side by side, four launches per step for all."""
    from .signnet import SIGNNetRuns as _c

    return _c(*args, **kwargs)


def LinkClassifier(*args, **kwargs):
    """See `s3grl_amd.linkclf.LinkClassifier`: sklearn's default LogisticRegression over emb[src] * emb[dst], solved by
    damped Newton on the GPU."""
    from .linkclf import LinkClassifier as _c

    return _c(*args, **kwargs)


def run_n2v(*args, **kwargs):
    """See `s3grl_amd.n2v.run_n2v` (reference baselines/n2v.run_n2v): the node2vec baseline on the GPU."""
    from .n2v import run_n2v as _f

    return _f(*args, **kwargs)


def run_n2v_row(*args, **kwargs):
    """See `s3grl_amd.n2v.run_n2v_row`: the Table 2 N2V row from a split."""
    from .n2v import run_n2v_row as _f

    return _f(*args, **kwargs)


def LinkMetrics(*args, **kwargs):
    """See `s3grl_amd.metrics.LinkMetrics`: AUC, AP, Hits@K and MRR of link scores, computed on the GPU."""
    from .metrics import LinkMetrics as _c

    return _c(*args, **kwargs)


def recommend_links(*args, **kwargs):
    """See `s3grl_amd.recommend.recommend`: the k most likely new links of every source node, on the GPU.  (The
    name `s3grl_amd.recommend` is the module.)"""
    from .recommend import recommend as _f

    return _f(*args, **kwargs)


def candidates(*args, **kwargs):
    """See `s3grl_amd.recommend.candidates`: per source, every node at graph distance 2..hops, on the GPU."""
    from .recommend import candidates as _f

    return _f(*args, **kwargs)


def segment_topk(*args, **kwargs):
    """See `s3grl_amd.recommend.segment_topk`: the k best scores of every segment, ties to the lower position."""
    from .recommend import segment_topk as _f

    return _f(*args, **kwargs)


def run_walkpool(*args, **kwargs):
    """See `s3grl_amd.walkpool.run_walkpool` (reference Software/WalkPooling/src/main.py): the Table 2 WalkPool row."""
    from .walkpool import run_walkpool as _f

    return _f(*args, **kwargs)


def WalkPoolSplit(*args, **kwargs):
    """See `s3grl_amd.walkpool.WalkPoolSplit`: E+ of a `SubgraphList` in both arc orders and its GCN operator."""
    from .walkpool import WalkPoolSplit as _c

    return _c(*args, **kwargs)


def LinkPredTwin(*args, **kwargs):
    """See `s3grl_amd.walkpool.LinkPredTwin`: WalkPool's model on HIP attention and walk-profile operators."""
    from .walkpool import LinkPredTwin as _c

    return _c(*args, **kwargs)
