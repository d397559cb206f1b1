"""DP-GSAT ("dual/primal") step: a second GSAT on the line graph steers the primal attention.

Restates ``GSAT.dual_forward_pass / __loss__ / f1_sparsity_loss / dual_train_one_batch / dual_eval_one_batch``
of the fork (src/run_gsat.py:121-180, 189-428, 612-637) on top of the HIP operators.  Not reproduced (SURVEY App. C,
marked X): the blocking ``input()`` / ``plt.show()`` / seaborn heat-maps, the host copies that only feed them
(:262-274) and the ``NameError`` on ``old_primal_edge_att`` in edge-attention mode (the unused ``comb_att`` is dropped).
Like the reference (:222) the dual attention is Gumbel-sampled in eval mode as well; ``gumbel_noise_in_eval=False`` opts into the
deterministic sigmoid(logits / tau).  The reference's ``assert`` on the ranges of p_uv / y_uv in ``f1_sparsity_loss`` (a host
sync per step) is not reproduced: both are outputs of a sigmoid / 0-1 labels by construction.
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .get_model import Criterion
from .ops import F1SparsityLoss, InfoLoss, Sample, edge_tensor
from .padding import padded
from .gsat import (concrete_sample, get_r, gumbel_sigmoid, info_loss, lift_node_att_to_edge_att,
                   symmetrise_edge_att)


def f1_sparsity_loss(p_uv, y_uv, eps=1e-6):
    """src/run_gsat.py:151-180: (1 - soft F1(p, y)) + mean|p|.  A handful of scalar reductions over [E]."""
    p, y = p_uv.view(-1), y_uv.view(-1)
    TP = (p * y).sum()
    P, G = p_uv.sum(), y_uv.sum()
    precision = TP / (P + eps)
    recall = TP / (G + eps)
    f1 = 2 * precision * recall / (precision + recall + eps)
    return (1 - f1) + p_uv.abs().mean()


def f1_sparsity_loss_valid(p, y, m_valid=None):
    """``f1_sparsity_loss`` as two HIP launches (one more for the backward) over the first ``m_valid`` entries -- one int32 on the device,
    e.g. ``batch.valid[1:2]`` of a padded batch; None counts every entry.  Entries beyond the count are not read (NaN there is harmless)
    and get a zero gradient; a count of 0 gives the loss 1 and zero gradients; ``y`` gets no gradient.  Bitwise repeatable and
    capturable into a hipGraph."""
    return F1SparsityLoss.apply(p, y.detach().float(), m_valid)


class DualGSAT(nn.Module):
    """The fork's two-model GSAT.  ``*_method_config``: pred_loss_coef, info_loss_coef, fix_r, decay_interval,
    decay_r, final_r, init_r (src/run_gsat.py:75-108); ``*_learn_edge_att`` from shared_config."""

    def __init__(self, primal_clf, primal_extractor, primal_optimizer, dual_clf, dual_extractor, dual_optimizer,
                 primal_method_config, dual_method_config, primal_learn_edge_att, dual_learn_edge_att,
                 primal_num_class=2, primal_multi_label=False, dual_num_class=2, dual_multi_label=False,
                 mix_alpha: float = 0.3, mix_after_epoch: int = 50, gumbel_tau: float = 0.1,
                 gumbel_noise_in_eval: bool = True):
        super().__init__()
        self.primal_clf, self.primal_extractor, self.primal_optimizer = primal_clf, primal_extractor, primal_optimizer
        self.dual_clf, self.dual_extractor, self.dual_optimizer = dual_clf, dual_extractor, dual_optimizer
        self.primal_learn_edge_att, self.dual_learn_edge_att = primal_learn_edge_att, dual_learn_edge_att
        self.primal_criterion = Criterion(primal_num_class, primal_multi_label)
        self.dual_criterion = Criterion(dual_num_class, dual_multi_label)
        for side, cfg in (("primal", primal_method_config), ("dual", dual_method_config)):
            setattr(self, side + "_pred_loss_coef", cfg["pred_loss_coef"])
            setattr(self, side + "_info_loss_coef", cfg["info_loss_coef"])
            setattr(self, side + "_fix_r", cfg.get("fix_r", None))
            setattr(self, side + "_decay_interval", cfg.get("decay_interval", None))
            setattr(self, side + "_decay_r", cfg.get("decay_r", None))
            setattr(self, side + "_final_r", cfg.get("final_r", 0.1))
            setattr(self, side + "_init_r", cfg.get("init_r", 0.9))
        self.mix_alpha, self.mix_after_epoch = mix_alpha, mix_after_epoch
        self.gumbel_tau, self.gumbel_noise_in_eval = gumbel_tau, gumbel_noise_in_eval
        self.sync_loss_dict = True
        self.keep_dual_att, self.dual_att = False, None      # ReplayedDualEval: keep the (detached) dual node attention of the last forward

    # -- src/run_gsat.py:121-149 -----------------------------------------------------------------------------------
    def __loss__(self, primal_att, dual_att, primal_clf_logits, dual_clf_logits, primal_clf_labels, dual_clf_labels,
                 dual_att_log_logits, epoch):
        primal_pred_loss = self.primal_criterion(primal_clf_logits, primal_clf_labels)
        dual_pred_loss = self.dual_criterion(dual_clf_logits, dual_clf_labels)
        dual_r = self.dual_fix_r if self.dual_fix_r else get_r(self.dual_decay_interval, self.dual_decay_r, epoch,
                                                                final_r=self.dual_final_r, init_r=self.dual_init_r)
        dual_info_loss = info_loss(dual_att, dual_r)
        primal_r = dual_att_log_logits.sigmoid().detach()                 # per-edge tensor prior (:129)
        primal_info_loss = info_loss(primal_att, primal_r)
        primal_pred_loss = primal_pred_loss * self.primal_pred_loss_coef
        primal_info_loss = primal_info_loss * self.primal_info_loss_coef
        dual_pred_loss = dual_pred_loss * self.dual_pred_loss_coef
        dual_info_loss = dual_info_loss * self.dual_info_loss_coef
        loss = primal_pred_loss + dual_pred_loss + primal_info_loss + dual_info_loss
        if self.sync_loss_dict:
            v = torch.stack([loss.detach(), dual_pred_loss.detach(), dual_info_loss.detach()]).tolist()
            loss_dict = {"loss": v[0], "pred": v[1], "info": v[2]}       # dual entries overwrite the primal ones (:145-146)
        else:
            loss_dict = {"loss": loss.detach(), "pred": dual_pred_loss.detach(), "info": dual_info_loss.detach()}
        return loss, loss_dict

    def _edge_att(self, att, data, learn_edge_att):
        if learn_edge_att:
            return symmetrise_edge_att(att, data.edge_index, data.x.shape[0])
        return lift_node_att_to_edge_att(att, data.edge_index)

    # -- src/run_gsat.py:189-428 -----------------------------------------------------------------------------------
    def dual_forward_pass(self, primal_data, dual_data, epoch, training, primal_noise=None, dual_noise=None,
                          primal_masks=None, dual_masks=None, dual_seed=None):
        """``dual_seed`` (an int, or a 1-element int64 ROCm tensor): where the dual Gumbel noise is drawn and ``dual_noise`` is None, draw
        it inside the sampler kernel from this seed (``gumbel_sigmoid(seed=)``) instead of from torch's generator."""
        from .graph_index import get_index
        if getattr(primal_data, "valid", None) is not None or getattr(dual_data, "valid", None) is not None:
            if getattr(primal_data, "pair", None) is not dual_data or getattr(dual_data, "pair", None) is not primal_data:
                raise ValueError("DualGSAT takes padded batches only as a pair from collate_padded_pair (whose primal edge slots and dual "
                                 "node rows line up): use it, or collate")
            return self._pair_forward_pass(primal_data, dual_data, epoch, training, primal_noise, dual_noise, primal_masks, dual_masks,
                                           dual_seed)
        for d in (primal_data, dual_data):
            if getattr(d, "num_graphs", None) is not None:      # prime the segment cache without `batch.max()` (a host sync)
                get_index(d.edge_index, d.x.shape[0]).graphs(d.batch, int(d.num_graphs))
        primal_emb = self.primal_clf.get_emb(primal_data.x, primal_data.edge_index, batch=primal_data.batch,
                                             edge_attr=primal_data.edge_attr)
        Mp = primal_data.edge_index.shape[1] if self.primal_learn_edge_att else primal_data.x.shape[0]
        if training and primal_noise is None:
            primal_noise = torch.empty(Mp, 1, device=primal_emb.device).uniform_(1e-10, 1 - 1e-10)
        _, primal_node_att = self.primal_extractor.attend(primal_emb, primal_data.edge_index, primal_data.batch,
                                                          primal_noise if training else None, primal_masks)
        dual_emb = self.dual_clf.get_emb(dual_data.x, dual_data.edge_index, batch=dual_data.batch, edge_attr=dual_data.edge_attr)
        dual_att_log_logits = self.dual_extractor(dual_emb, dual_data.edge_index, dual_data.batch, dropout_masks=dual_masks)
        if training or self.gumbel_noise_in_eval:
            dual_node_att = gumbel_sigmoid(dual_att_log_logits, tau=self.gumbel_tau, noise=dual_noise, seed=dual_seed)       # :222
        else:
            dual_node_att = Sample.apply(dual_att_log_logits, None, 0, self.gumbel_tau, 0.0)   # sigmoid(logits / tau), no noise
        if self.keep_dual_att:
            self.dual_att = dual_node_att.detach()
        y_uv = primal_data.edge_label.float().to(dual_node_att.device)
        f1_loss = f1_sparsity_loss(dual_node_att, y_uv)                                                       # :226-227
        dual_edge_att = self._edge_att(dual_node_att, dual_data, self.dual_learn_edge_att)                     # :231-239
        primal_edge_att = self._edge_att(primal_node_att, primal_data, self.primal_learn_edge_att)             # :241-250
        if epoch > self.mix_after_epoch:                                                                      # :252-253
            primal_edge_att = self.mix_alpha * dual_node_att + (1 - self.mix_alpha) * primal_edge_att
        primal_clf_logits = self.primal_clf(primal_data.x, primal_data.edge_index, primal_data.batch,
                                            edge_attr=primal_data.edge_attr, edge_atten=primal_edge_att)
        dual_clf_logits = self.dual_clf(dual_data.x, dual_data.edge_index, dual_data.batch,
                                        edge_attr=dual_data.edge_attr, edge_atten=dual_edge_att)
        loss, loss_dict = self.__loss__(primal_edge_att, dual_edge_att, primal_clf_logits, dual_clf_logits,
                                        primal_data.y, dual_data.y, dual_att_log_logits, epoch)                # :276
        loss = loss + f1_loss                                                                                 # :281
        return primal_edge_att, loss, loss_dict, primal_clf_logits

    def _pair_forward_pass(self, pb, db, epoch, training, primal_noise, dual_noise, primal_masks, dual_masks, dual_seed=None):
        """``dual_forward_pass`` on a padded pair (collate_padded_pair): dual node row k < Ep is primal edge slot k.  Every primal module runs
        inside ``padded(pb.valid)``, every dual one inside ``padded(db.valid)``; the whole-batch reductions take their counts from the
        device (f1 and the primal info loss: pb.valid[1]; the dual info loss: db.valid[1], with ``db.r`` -- one device float, when set --
        as its r); both criteria see the real graphs ``[:B]`` -- of a ragged pair (``collate_padded_pair(..., ragged=True)``) the ``B`` graph
        slots, of which they read the filled count ``pb.valid[2]`` on the device (``criterion_valid``).  No host decision depends on the
        batch, so the call can be captured; every output has capacity shape."""
        from .graph_index import get_index
        if self.primal_learn_edge_att or self.dual_learn_edge_att:
            raise ValueError("a padded pair takes node attention on both sides (the MUTAG configs), not edge attention")
        if self.primal_criterion.multi_label or self.dual_criterion.multi_label:
            raise ValueError("a padded batch cannot take the multi-label criterion (its boolean indexing is not capturable)")
        if pb.edge_label is None:
            raise ValueError("the f1 sparsity loss needs the primal dataset's edge_label")
        (Np, Ep), (Nd, Ed) = pb.capacity, db.capacity
        B = int(pb.num_graphs) - 1
        if Nd != Ep + 2 or int(db.num_graphs) - 1 != B:
            raise ValueError("not a padded pair: the dual node capacity must be the primal edge capacity + 2, with the same graphs")
        ragged = bool(getattr(pb, "ragged", False))
        if ragged != bool(getattr(db, "ragged", False)):
            raise ValueError("not a padded pair: one side is ragged and the other is not (collate_padded_pair(..., ragged=True) makes both)")
        g_valid = pb.valid[2:3] if ragged else None          # filled slots (= db.valid[2:3]), read by the criterion kernel
        pctx, dctx = (lambda: padded(pb.valid, pb.capacity)), (lambda: padded(db.valid, db.capacity))
        for d in (pb, db):
            get_index(d.edge_index, d.x.shape[0]).graphs(d.batch, int(d.num_graphs))
        with pctx():
            primal_emb = self.primal_clf.get_emb(pb.x, pb.edge_index, batch=pb.batch, edge_attr=pb.edge_attr)
            if training and primal_noise is None:
                primal_noise = torch.empty(Np, 1, device=primal_emb.device).uniform_(1e-10, 1 - 1e-10)
            _, primal_node_att = self.primal_extractor.attend(primal_emb, pb.edge_index, pb.batch, primal_noise if training else None,
                                                              primal_masks)
        with dctx():
            dual_emb = self.dual_clf.get_emb(db.x, db.edge_index, batch=db.batch, edge_attr=db.edge_attr)
            dual_att_log_logits = self.dual_extractor(dual_emb, db.edge_index, db.batch, dropout_masks=dual_masks)
        if training or self.gumbel_noise_in_eval:
            dual_node_att = gumbel_sigmoid(dual_att_log_logits, tau=self.gumbel_tau, noise=dual_noise, seed=dual_seed)
        else:
            dual_node_att = Sample.apply(dual_att_log_logits, None, 0, self.gumbel_tau, 0.0)
        if self.keep_dual_att:
            self.dual_att = dual_node_att.detach()
        n_edges = pb.valid[1:2]                                                  # = db.valid[0:1]: the real primal edges / dual nodes
        dual_on_edges = dual_node_att[:Ep]
        f1_loss = f1_sparsity_loss_valid(dual_on_edges, pb.edge_label, n_edges)
        dual_edge_att = lift_node_att_to_edge_att(dual_node_att, db.edge_index)
        primal_edge_att = lift_node_att_to_edge_att(primal_node_att, pb.edge_index)
        if epoch > self.mix_after_epoch:
            primal_edge_att = self.mix_alpha * dual_on_edges + (1 - self.mix_alpha) * primal_edge_att
        with pctx():
            primal_clf_logits = self.primal_clf(pb.x, pb.edge_index, pb.batch, edge_attr=pb.edge_attr, edge_atten=primal_edge_att)
        with dctx():
            dual_clf_logits = self.dual_clf(db.x, db.edge_index, db.batch, edge_attr=db.edge_attr, edge_atten=dual_edge_att)
        # __loss__ with counts: the same terms, coefficients, order of the sum and loss dict -- change the two together
        primal_pred_loss = self.primal_criterion(primal_clf_logits[:B], pb.y[:B], g_valid=g_valid) * self.primal_pred_loss_coef
        dual_pred_loss = self.dual_criterion(dual_clf_logits[:B], db.y[:B], g_valid=g_valid) * self.dual_pred_loss_coef
        dual_r = self.dual_fix_r if self.dual_fix_r else get_r(self.dual_decay_interval, self.dual_decay_r, epoch,
                                                                final_r=self.dual_final_r, init_r=self.dual_init_r)
        dual_info_loss = InfoLoss.apply(edge_tensor(dual_edge_att), dual_r, db.valid[1:2], getattr(db, "r", None)) * self.dual_info_loss_coef
        prior = dual_att_log_logits.sigmoid().detach()[:Ep]
        primal_info_loss = InfoLoss.apply(edge_tensor(primal_edge_att), prior, n_edges, None) * self.primal_info_loss_coef
        loss = primal_pred_loss + dual_pred_loss + primal_info_loss + dual_info_loss
        if self.sync_loss_dict:
            v = torch.stack([loss.detach(), dual_pred_loss.detach(), dual_info_loss.detach()]).tolist()
            loss_dict = {"loss": v[0], "pred": v[1], "info": v[2]}
        else:
            loss_dict = {"loss": loss.detach(), "pred": dual_pred_loss.detach(), "info": dual_info_loss.detach()}
        return primal_edge_att, loss + f1_loss, loss_dict, primal_clf_logits

    # -- src/run_gsat.py:612-637 -----------------------------------------------------------------------------------
    def dual_train_one_batch(self, primal_data, dual_data, epoch):
        for m in (self.primal_extractor, self.primal_clf, self.dual_extractor, self.dual_clf):
            m.train()
        att, loss, loss_dict, clf_logits = self.dual_forward_pass(primal_data, dual_data, epoch, training=True)
        self.primal_optimizer.zero_grad()
        self.dual_optimizer.zero_grad()
        loss.backward()
        self.primal_optimizer.step()
        self.dual_optimizer.step()
        return att.data.cpu().reshape(-1), loss_dict, clf_logits.data.cpu()

    @torch.no_grad()
    def dual_eval_one_batch(self, primal_data, dual_data, epoch):
        for m in (self.primal_extractor, self.primal_clf, self.dual_extractor, self.dual_clf):
            m.eval()
        att, loss, loss_dict, clf_logits = self.dual_forward_pass(primal_data, dual_data, epoch, training=False)
        return att.data.cpu().reshape(-1), loss_dict, clf_logits.data.cpu()
