"""DDI evaluation on the device: madrigal/evaluate/evaluate.py:147-247 (evaluate_ddi).

The reference runs the dense [L,N,N] forward, copies it to the host (evaluate.py:191), gathers the labelled triples there and
calls sklearn once per outcome.  Here the plan of the labelled triples (``ops.triple_plan``) feeds ``model.score_triples``, which
computes only those logits, in the triples' original order; the loss and ``metrics.get_metrics`` run on the device, and only the
[13, L] metric table and the loss reach the host.  Out of scope: ONSIDES single-drug mode and ``save_scores`` (per-label output)."""
from __future__ import annotations

import torch

from . import masks as MK
from . import metrics as MT
from . import ops

KEY_METRIC = {"multilabel": "auprc", "multiclass": "auprc"}        # eval_utils.py KEY_METRIC_DICT
_SYMMETRIC_TYPES = {"str_str", "full_full", "kg_kg", "cv_cv", "tx_tx"}
_WITHIN_SPLITS = {"val", "val_within", "val_within_easy", "test", "test_within", "test_within_easy"}
_BETWEEN_SPLITS = {"val_between", "val_between_easy", "test_between", "test_between_easy"}


def direct_triples(ddi_head_indices, ddi_tail_indices, ddi_labels, ddi_pos_neg_samples, eval_type: str, split: str):
    """The direction rules (1)-(3) of evaluate.py:161-187 -> (heads, tails, labels, targets)."""
    head_kind, tail_kind = eval_type.split("_")
    if split == "train" and eval_type in _SYMMETRIC_TYPES:          # (1) train triples were made bidirectional: keep one direction
        keep = ddi_head_indices < ddi_tail_indices
        return ddi_head_indices[keep], ddi_tail_indices[keep], ddi_labels[keep], ddi_pos_neg_samples[keep]
    if split in _WITHIN_SPLITS and head_kind != tail_kind:          # (2) asymmetric eval type: score both directions
        return (torch.cat([ddi_head_indices, ddi_tail_indices]), torch.cat([ddi_tail_indices, ddi_head_indices]), ddi_labels.repeat(2),
                ddi_pos_neg_samples.repeat(2))
    return ddi_head_indices, ddi_tail_indices, ddi_labels, ddi_pos_neg_samples   # (3) between splits, train str_full, the rest


@torch.no_grad()
def evaluate_ddi(model, batch_head, batch_tail, batch_kg, head_masks_base, tail_masks_base, ddi_head_indices, ddi_tail_indices, ddi_labels,
                 ddi_pos_neg_samples, loss_fn, k, task, eval_type, split, finetune_mode, best_metrics, verbose=True, logger=None, wandb=None,
                 epoch=None, data_source="", return_all=False, **model_kwargs):
    """Drop-in for evaluate.py:evaluate_ddi on the HIP path -> the key metric (``auprc``); with ``return_all`` also the macro metric
    dict, the loss and the scored triples: ``(key_metric, metrics_dict, loss, triples)`` with ``triples`` a dict of the device
    tensors ``pred`` (probabilities), ``labels``, ``heads``, ``tails``, ``targets`` after the direction rules.  ``batch_head`` / ``batch_tail`` / ``batch_kg`` are on the model's device;
    the index and target tensors may be anywhere.  ``model_kwargs`` go to ``model.score_triples`` (e.g. ``kg_filler``)."""
    if len(eval_type.split("_")) != 2:
        raise AssertionError(f"eval_type must be '<head>_<tail>', got {eval_type!r}")
    if "ONSIDES" in data_source:
        raise NotImplementedError("evaluate_ddi: the ONSIDES single-drug mode is not implemented on the HIP path")
    if task not in KEY_METRIC:
        raise ValueError(f"evaluate_ddi: task must be one of {sorted(KEY_METRIC)}, got {task!r}")
    dev = next(model.parameters()).device
    masks_head, masks_tail = MK.get_evaluate_masks(head_masks_base, tail_masks_base, eval_type, finetune_mode, dev)
    heads, tails, labels, targets = direct_triples(ddi_head_indices, ddi_tail_indices, ddi_labels, ddi_pos_neg_samples, eval_type, split)
    heads, tails, labels = (t.to(dev, torch.int64) for t in (heads, tails, labels))
    targets = targets.to(dev, torch.float32)
    model.eval()
    n_labels = int(model.decoder.out_features)
    plan = ops.triple_plan(labels, heads, tails, n_labels, masks_head.shape[0], masks_tail.shape[0])
    pred = torch.sigmoid(model.score_triples(batch_head, batch_tail, masks_head, masks_tail, batch_kg, plan, **model_kwargs))
    loss = loss_fn(pred, targets).item()
    if logger is not None:
        logger.info(f"Evaluated for {task} classification task on {split} set with {eval_type} eval_type.")
    metrics_dict, _ = MT.get_metrics(pred, targets, labels, k=k, task=task, logger=logger, average="macro", verbose=verbose)
    if logger is not None:
        logger.info(f"{data_source}{split}_{eval_type}_loss: {loss:.4f}")
    if wandb is not None:
        wandb.log({f"{data_source}{split}_{eval_type}_loss": loss}, step=epoch)
        wandb.log({f"{data_source}{split}_{eval_type}_{name}": v if v == v else 0 for name, v in metrics_dict.items()}, step=epoch)
    key_name = KEY_METRIC[task]
    key_metric = metrics_dict[key_name]
    best_key = f"{data_source}best_{split}_{eval_type}_{key_name}"
    if best_metrics is not None and (best_key not in best_metrics or key_metric > best_metrics[best_key]):
        for name, v in metrics_dict.items():
            best_metrics[f"{data_source}best_{split}_{eval_type}_{name}"] = v
    if return_all:
        return key_metric, metrics_dict, loss, dict(pred=pred, labels=labels, heads=heads, tails=tails, targets=targets)
    return key_metric
