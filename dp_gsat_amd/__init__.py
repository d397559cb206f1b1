"""dp_gsat_amd -- MI355X (gfx950) implementation of GSAT's edge-attention + stochastic mask + masked
message-passing hot path behind the reference's PyG-style operator surface.

Public names follow the reference: ``get_model, GIN, PNA, GINConv, GINEConv, PNAConvSimple, MLP,
ExtractorMLP, GSAT, Criterion, get_preds, reorder_like, process_data``.
Everything computes through ``libgsat_hip.so`` (C ABI: include/gsat_hip.h); there is no CPU fallback.
"""
from .get_model import MLP, BatchSequential, Criterion, InstanceNorm, criterion_valid, get_model, get_preds
from .conv_layers import GINConv, GINEConv, LEConv, PNAConvSimple
from .gin import GIN
from .pna import PNA
from .spmotif_gnn import SPMotifNet
from .gsat import (GSAT, ExtractorMLP, concrete_sample, get_r, gumbel_sigmoid, info_loss,
                   lift_node_att_to_edge_att, symmetrise_edge_att)
from .collate import PackedDataset, PaddedBatch, collate_padded_pair, line_graph, line_graph_undirected
from .padding import current_padding, padded
from .replay import ReplayedDualEval, ReplayedDualStep, ReplayedEval, ReplayedFidelity, ReplayedFidelityCurve, ReplayedStep
from .dual_gsat import DualGSAT, f1_sparsity_loss, f1_sparsity_loss_valid
from .graph_index import BatchIndex, clear_cache, get_index, set_strict, set_sync_free
from .utils import process_data, reorder_like, set_seed
from .explain import EdgeRanking, ExplanationMeter, attention_auroc, delta_kl, precision_at_k, rank_edges, topk_edge_mask
from .explain import explanation_levels
from .subgraph import (PaddedSubgraphBatch, SubgraphBatch, edge_subgraph, edge_subgraph_padded, explanation_fidelity, explanation_subgraph,
                       gather_rows, node_subgraph, node_subgraph_padded)
from .subgraph import StackedExplanationBatch, explanation_fidelity_curve, explanation_stack
from .subgraph import explanation_fidelity_curves, explanation_stack_multi
from .explain import level_overlap
from .replay import ReplayedDualFidelityCurve
from .explain import NodeRanking, node_levels, node_precision_at_k, rank_nodes, topk_node_mask
from .subgraph import explanation_node_fidelity_curve, explanation_node_subgraph, explanation_stack_nodes
from .evaluate import (AttentionHistogram, EvaluationMeter, attention_histogram, classifier_accuracy, classifier_rocauc, classifier_rocauc_tasks, pr_curve,
                       task_auroc_counts)
from .eval_log import EpochLog, FidelityCurveLog, FidelityLog, delta_kl_segments
from .eval_log import ClfLog
from .replay import ReplayedClfEval, ReplayedClfStep
from .pretrain import pretrain_clf, update_best_clf
from .explain import (LevelComponents, component_labels, components_lds_cap, explanation_connectivity, largest_component_mask, level_components,
                      level_components_reset)
from .baselines import Explanation, GNNExplainer, MaskState, edge_saliency, normalise_per_graph
from .replay import ReplayedGNNExplainer

__all__ = ["MLP", "BatchSequential", "Criterion", "InstanceNorm", "get_model", "get_preds", "GINConv", "GINEConv",
           "PNAConvSimple", "GIN", "PNA", "GSAT", "ExtractorMLP", "concrete_sample", "get_r", "gumbel_sigmoid",
           "info_loss", "lift_node_att_to_edge_att", "symmetrise_edge_att", "BatchIndex", "get_index", "clear_cache", "set_sync_free", "set_strict",
           "process_data", "reorder_like", "set_seed", "DualGSAT", "f1_sparsity_loss", "LEConv", "SPMotifNet", "PackedDataset", "line_graph", "line_graph_undirected",
           "EdgeRanking", "ExplanationMeter", "attention_auroc", "delta_kl", "precision_at_k", "rank_edges", "topk_edge_mask",
           "SubgraphBatch", "edge_subgraph", "node_subgraph", "explanation_subgraph", "explanation_fidelity", "gather_rows",
           "AttentionHistogram", "EvaluationMeter", "attention_histogram", "classifier_accuracy", "classifier_rocauc", "classifier_rocauc_tasks", "pr_curve",
           "task_auroc_counts", "PaddedBatch", "padded", "current_padding", "ReplayedStep",
           "ReplayedDualStep", "collate_padded_pair", "f1_sparsity_loss_valid", "EpochLog", "delta_kl_segments", "ReplayedEval",
           "ReplayedDualEval", "criterion_valid", "PaddedSubgraphBatch", "edge_subgraph_padded", "node_subgraph_padded", "FidelityLog", "ReplayedFidelity",
           "explanation_levels", "StackedExplanationBatch", "explanation_stack", "explanation_fidelity_curve", "FidelityCurveLog",
           "ReplayedFidelityCurve", "explanation_stack_multi", "explanation_fidelity_curves", "level_overlap",
           "ReplayedDualFidelityCurve", "NodeRanking", "rank_nodes", "topk_node_mask", "node_levels", "node_precision_at_k",
           "explanation_node_subgraph", "explanation_stack_nodes", "explanation_node_fidelity_curve",
           "ClfLog", "ReplayedClfStep", "ReplayedClfEval", "pretrain_clf", "update_best_clf", "LevelComponents", "components_lds_cap",
           "level_components", "level_components_reset", "largest_component_mask", "component_labels", "explanation_connectivity",
           "GNNExplainer", "Explanation", "MaskState", "edge_saliency", "normalise_per_graph", "ReplayedGNNExplainer"]
