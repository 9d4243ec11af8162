"""DDI evaluation on the device: madrigal/evaluate/evaluate.py:147-247 (evaluate_ddi).

The reference runs the dense [L,N,N] forward, copies it to the host (evaluate.py:191), gathers the labelled triples there and
calls sklearn once per outcome.  Here the plan of the labelled triples (``ops.triple_plan``) feeds ``model.score_triples``, which
computes only those logits, in the triples' original order; the loss and ``metrics.get_metrics`` run on the device, and only the
[13, L] metric table and the loss reach the host.  Out of scope: ONSIDES single-drug mode and ``save_scores`` (per-label output)."""
from __future__ import annotations

import numpy as np
import torch

from . import data as D
from . import masks as MK
from . import metrics as MT
from . import ops
from . import retrieval as RT

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


# ------------------------------------------------------------------------------------------------- pretraining evaluation
# madrigal/evaluate/evaluate.py:250-403 (evaluate_pt, evaluate_pretrain_subsets).  The reference runs the CL head through
# model.cpu() (evaluate.py:395-397), which our model classes cannot do, and its metrics in CPU torch on a random subsample of
# at most 1000 drugs (evaluate.py:365-366).  Here the encoder, the CL head and every metric run on the model's device
# (retrieval.py, csrc/retrieval.hip); only the final scalars reach the host.  ``max_drugs=None`` evaluates every valid drug: the
# CL-head loss (ops.info_nce through ``model(...)``) then materialises the [2n,2n] similarities and the [2n,2n-1] logits and
# labels, about 6.5 GB at n = 11 607.
MODALITY2NUMBER_LIST = dict({m: [i] for i, m in enumerate(D.NON_TX_MODALITIES)},
                            **{f"tx_{c}": [i + D.NUM_NON_TX_MODALITIES] for i, c in enumerate(D.CELL_LINES)})
NUMBER2MODALITY = {str(v[0]): k for k, v in MODALITY2NUMBER_LIST.items()}
PT_PAIRS = ["kg", "cv"] + (["bs"] if D.NUM_NON_TX_MODALITIES > 3 else []) + ["tx_mcf7", "tx_pc3", "tx_vcap"]
PT_UNIFORMITY_MODALITIES = ["str", "kg", "cv"] + (["bs"] if D.NUM_NON_TX_MODALITIES > 3 else []) + ["tx_mcf7", "tx_pc3", "tx_vcap"]


def from_indices_to_tensor(indices, size) -> torch.Tensor:
    """madrigal/utils.py:398-409 with its defaults (value 0 at ``indices``, 1 elsewhere, last dim)."""
    idx = indices if isinstance(indices, torch.Tensor) else torch.tensor(indices)
    return torch.ones(size).scatter(dim=-1, index=idx, value=0)


def pretrain_subset_keys(split: str, comp_pair: str) -> list:
    """The 14 report keys of evaluate_pt (evaluate.py:266-277) for one pair, in the order of evaluate_pretrain_subsets' tuple."""
    keys = [f"{split} {topk} acc {comp_pair} {embed_type} {side_type} (cosine)"
            for side_type in ("one-side", "both-side") for embed_type in ("embed", "CL-head") for topk in ("top20", "top5", "top1")]
    return keys + [f"{split} loss {comp_pair}", f"{split} foscttm mu {comp_pair}"]


def pretrain_log_keys(split: str) -> list:
    """Every key evaluate_pt logs, grouped by wandb.log call: [report keys], then one uniformity key per modality, then one
    alignment key per pair."""
    report = sum((pretrain_subset_keys(split, f"str v {m}") for m in PT_PAIRS), [])
    uni = [[f"{split} uniformity loss {m}"] for m in PT_UNIFORMITY_MODALITIES]
    ali = [[f"{split} alignment loss str v {m}"] for m in PT_PAIRS]
    return [report] + uni + ali


def _to(x, device):
    """utils.to_device for the collator's output: tensors and objects with ``.to`` move, numpy arrays and the rest stay."""
    if isinstance(x, dict):
        return {k: _to(v, device) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_to(v, device) for v in x]
    if isinstance(x, torch.Tensor) or (hasattr(x, "to") and not isinstance(x, np.ndarray)):
        return x.to(device)
    return x


def _subset_masks(subset, n_rows: int, n_cols: int, device) -> torch.Tensor:
    return from_indices_to_tensor(subset, n_cols).repeat(n_rows, 1).bool().to(device)


def _encode(model, drug_ids: torch.Tensor, subset, data, n_cols: int, device) -> torch.Tensor:
    mols, kg, cv, tx = data
    m = _subset_masks(subset, drug_ids.shape[0], n_cols, device)
    return model.base_encoder(drug_ids, m, mols, kg, cv, tx, raw_encoder_output=model.raw_encoder_output)


def _valid_drugs(drugs: np.ndarray, masks: np.ndarray, cols) -> np.ndarray:
    return drugs[(1 - masks[drugs, :][:, cols]).sum(axis=1) == len(cols)]


@torch.no_grad()
def evaluate_pretrain_subsets(model, drugs, masks, too_hard_neg_mask, collator, subset1, subset2, device, max_drugs=1000):
    """Drop-in for evaluate.py:360-403 -> the reference's 14-tuple: top20 / top5 / top1 one-side accuracies of the embeddings
    and of the CL-head outputs, the same six stacked (both-side), the CL-head loss and the mean FOSCTTM of both directions.
    The 12 accuracies are Python floats; ``loss`` and ``foscttm_mu`` are 0-dim CPU tensors.

    Drugs owning every modality of subset1 + subset2 are kept as at evaluate.py:364, and ``np.random.choice(valid, min(max_drugs,
    len(valid)), replace=False)`` draws from numpy's global generator exactly where the reference draws (a seeded run evaluates
    the same drugs).  ``max_drugs=None`` takes every valid drug in order and draws nothing.  Fewer than 20 valid drugs raise
    ValueError (the reference's topk(20) raises).  The CL head runs on the model's device (the reference moves the model to the
    CPU).  Ties count as hits (retrieval.py)."""
    cols = np.unique(list(subset1) + list(subset2))
    valid = _valid_drugs(np.asarray(drugs), np.asarray(masks), cols)
    if max_drugs is not None:
        valid = np.random.choice(valid, size=min(int(max_drugs), valid.shape[0]), replace=False)
    if valid.shape[0] < 20:
        raise ValueError(f"evaluate_pretrain_subsets: {valid.shape[0]} valid drugs for subsets {list(subset1)} / {list(subset2)}; "
                         "the top-20 metrics need at least 20")
    dev = next(model.parameters()).device
    valid_t = torch.from_numpy(np.asarray(valid, dtype=np.int64))
    _, valid_data = collator([valid_t])
    valid_data = _to(valid_data, dev)
    ids = valid_t.to(dev)
    n_cols = int(np.asarray(masks).shape[1])
    e1 = _encode(model, ids, subset1, valid_data, n_cols, dev)
    e2 = _encode(model, ids, subset2, valid_data, n_cols, dev)
    ce = RT.pair_counts(e1, e2)
    if too_hard_neg_mask is not None:
        hard = too_hard_neg_mask if isinstance(too_hard_neg_mask, torch.Tensor) else torch.from_numpy(np.asarray(too_hard_neg_mask))
        hard = hard[valid_t, :][:, valid_t].to(dev)
    else:
        hard = None
    m1, m2 = (_subset_masks(s, ids.shape[0], n_cols, dev) for s in (subset1, subset2))
    aug1, aug2, (_, _, loss) = model(ids, m1, m2, hard, valid_data, None, None)
    ch = RT.pair_counts(aug1, aug2)
    ks = [("one", k) for k in (20, 5, 1)] + [("both", k) for k in (20, 5, 1)]
    a_e, a_h = RT.topk_from_counts(ce, ks), RT.topk_from_counts(ch, ks)
    n = int(ids.shape[0])
    f1 = RT.topk_fraction(ce["dist_col"], n)                    # foscttm(embeds1, embeds2)
    f2 = RT.topk_fraction(ce["dist_row"], n)                    # foscttm(embeds2, embeds1)
    mu = (f1.mean() + f2.mean()) / 2
    accs = [a_e[("one", k)] for k in (20, 5, 1)] + [a_h[("one", k)] for k in (20, 5, 1)] + \
           [a_e[("both", k)] for k in (20, 5, 1)] + [a_h[("both", k)] for k in (20, 5, 1)]
    host = torch.stack(accs + [loss.reshape(()).to(torch.float32), mu]).cpu()       # the one device-to-host copy of the results
    vals = host.tolist()
    return tuple(vals[:12]) + (host[12].clone(), host[13].clone())


@torch.no_grad()
def evaluate_pt(model, drugs, masks, too_hard_neg_mask, collator, split, wandb, logger, device, epoch, max_drugs=1000):
    """Drop-in for evaluate.py:250-357 on the HIP path: evaluate_pretrain_subsets for str v kg / cv / tx_mcf7 / tx_pc3 / tx_vcap
    (one wandb.log of the report dict), uniformity over every valid drug of each modality, alignment over the shared drugs sorted
    by drug id; the same wandb.log calls and keys as the reference, with ``step=epoch``.  Returns the reference's
    ``all_embeds``: {str(col): {'embeds': CPU tensor, 'drugs': np.ndarray}}.  ``max_drugs`` goes to evaluate_pretrain_subsets."""
    dev = next(model.parameters()).device
    drugs, masks = np.asarray(drugs), np.asarray(masks)
    report = {}
    for m in PT_PAIRS:
        comp_pair = f"str v {m}"
        vals = evaluate_pretrain_subsets(model, drugs, masks, too_hard_neg_mask, collator, MODALITY2NUMBER_LIST["str"],
                                         MODALITY2NUMBER_LIST[m], device, max_drugs=max_drugs)
        report.update(zip(pretrain_subset_keys(split, comp_pair), vals))
    wandb.log(report, step=epoch)
    if logger is not None:
        logger.info("Start logging uniformity metrics...")
    all_embeds, dev_embeds = {}, {}
    for name in PT_UNIFORMITY_MODALITIES:
        mod = MODALITY2NUMBER_LIST[name][0]
        valid = _valid_drugs(drugs, masks, [mod])
        valid_drugs, valid_data = collator([valid])
        valid_drugs = torch.as_tensor(valid_drugs)
        valid_data = _to(valid_data, dev)
        embeds = _encode(model, valid_drugs.to(dev), [mod], valid_data, masks.shape[1], dev)
        uniform_l = RT.uniform_loss(embeds).cpu()
        wandb.log({f"{split} uniformity loss {name}": uniform_l}, step=epoch)
        if logger is not None:
            logger.info(f"{split} uniformity loss {name}: {uniform_l}")
        dev_embeds[str(mod)] = embeds
        all_embeds[str(mod)] = {"embeds": embeds.cpu(), "drugs": valid_drugs.detach().cpu().numpy()}
    if logger is not None:
        logger.info("Start logging alignment metrics...")
    for name in PT_PAIRS:
        mod1, mod2 = 0, MODALITY2NUMBER_LIST[name][0]
        d1, d2 = all_embeds[str(mod1)]["drugs"], all_embeds[str(mod2)]["drugs"]
        shared = np.intersect1d(d1, d2)
        sel = []
        for d in (d1, d2):
            keep = np.isin(d, shared)
            pos = np.nonzero(keep)[0][np.argsort(d[keep])]                  # evaluate.py:330-351: shared drugs sorted by id
            sel.append(torch.from_numpy(pos).to(dev))
        alignment_l = RT.alignment_loss(dev_embeds[str(mod1)].index_select(0, sel[0]), dev_embeds[str(mod2)].index_select(0, sel[1])).cpu()
        wandb.log({f"{split} alignment loss str v {name}": alignment_l}, step=epoch)
        if logger is not None:
            logger.info(f"{split} alignment loss str v {name}: {alignment_l}")
    return all_embeds


# ------------------------------------------------------------------------------------------------- final embeddings: GeomCA
# madrigal/evaluate/evaluate.py:456-504 (evaluate_final_embeds, get_alignment_metrics) on the ``all_embeds`` dicts of evaluate_pt.
# The reference stacks the shared drugs' rows on the host and runs GeomCA through GUDHI and networkx; here ``retrieval.geomca``
# runs on the device.  ``save_dir`` is accepted and nothing is written: no plots, pickles or logs.
def get_alignment_metrics(pair_name, outputs_subset1, outputs_subset2, save_dir, wandb, logger, epoch, parameters=None):
    """Drop-in for evaluate.py:464-504: GeomCA of the two modalities' embeddings over their shared drugs (``np.intersect1d``:
    sorted by drug id), one ``wandb.log`` of precision, recall, network consistency, network quality and sample size with
    ``step=epoch``.  ``outputs_subset*``: {'embeds': CPU or CUDA tensor [n,128], 'drugs': ids [n]}.  ``parameters`` overrides
    ``retrieval.GEOMCA_DEFAULTS``.  Returns GeomCA's ``(comp_stats, network_stats, network_params)`` (the reference returns None)."""
    drugs1, drugs2 = np.asarray(outputs_subset1["drugs"]), np.asarray(outputs_subset2["drugs"])
    pos1 = {d: i for i, d in enumerate(drugs1.tolist())}
    pos2 = {d: i for i, d in enumerate(drugs2.tolist())}
    valid_drugs = np.intersect1d(drugs1, drugs2)
    if valid_drugs.size == 0:
        raise ValueError(f"get_alignment_metrics: {pair_name}: the two subsets share no drug")
    rows = []
    for embeds, pos in ((outputs_subset1["embeds"], pos1), (outputs_subset2["embeds"], pos2)):
        embeds = torch.as_tensor(embeds)
        sel = torch.tensor([pos[d] for d in valid_drugs.tolist()], dtype=torch.int64, device=embeds.device)
        rows.append(embeds.index_select(0, sel))
    results = RT.geomca(rows[0], rows[1], **(parameters or {}))
    net = results[1]
    wandb.log({f"{pair_name} GeomCA precision": net["precision"], f"{pair_name} GeomCA recall": net["recall"],
               f"{pair_name} GeomCA network consistency": net["network_consistency"],
               f"{pair_name} GeomCA network quality": net["network_quality"], f"{pair_name} GeomCA sample size": len(valid_drugs)},
              step=epoch)
    if logger is not None:
        logger.info(f"GeomCA evaluation...\n{pair_name} precision: {net['precision']}, recall: {net['recall']}, network consistency: "
                    f"{net['network_consistency']}, network quality: {net['network_quality']}, sample size: {len(valid_drugs)}")
    return results


def evaluate_final_embeds(train_outputs, val_outputs, save_dir, wandb, logger, epoch):
    """Drop-in for evaluate.py:456-461: ``get_alignment_metrics`` for every pair of modalities of the train and of the val
    ``all_embeds`` dict (``evaluate_pt``'s return value), named 'train <m1> v <m2>' / 'val <m1> v <m2>'."""
    from itertools import combinations
    for split, outputs in (("train", train_outputs), ("val", val_outputs)):
        for (key1, subset1), (key2, subset2) in combinations(outputs.items(), 2):
            get_alignment_metrics(f"{split} {NUMBER2MODALITY[key1]} v {NUMBER2MODALITY[key2]}", subset1, subset2, save_dir, wandb, logger, epoch)
