"""Predictions of a finetuned checkpoint and the drug-stratified scores: madrigal/evaluate/predict.py:173-241 (make_predictions) and
:274-355 (get_drug_specific_scores).

The reference runs the dense [L,N,N] forward, copies it to the host and gathers the labelled triples there; its per-drug scores
then call sklearn's get_metrics once per drug and label.  Here the labelled triples are scored alone (``ops.triple_plan`` +
``model.score_triples``, as ``evaluate.evaluate_ddi`` does), and ``metrics.drug_specific_metrics`` computes every drug's metrics in
one ``ops.group_metrics`` call.  Out of scope: ``force_ori_modalities`` (the reference's temporary three-modality rebuild)."""
from __future__ import annotations

import torch

from . import checkpoint as CK
from . import masks as MK
from . import metrics as MT
from . import ops
from .evaluate import _to


def _model(ckpt_or_checkpoint_dir, device):
    from .models import NovelDDIMultilabel
    if isinstance(ckpt_or_checkpoint_dir, NovelDDIMultilabel):
        return ckpt_or_checkpoint_dir.to(device)
    path = str(ckpt_or_checkpoint_dir)
    path = path if path.endswith(".pt") else path + "best_model.pt"          # the reference's naming (predict.py:178-181)
    model, _, _ = CK.load_finetune_checkpoint(path, device=device, strict=False)
    return model


def _scores(model, batch, eval_type, finetune_mode, device, return_all_pairwise, **model_kwargs):
    model.eval()
    bh, bt, bkg = (_to(batch[s], device) for s in ("head", "tail", "kg"))
    mh, mt = MK.get_evaluate_masks(batch["head"]["masks"], batch["tail"]["masks"], eval_type, finetune_mode, device)
    if return_all_pairwise:
        return torch.sigmoid(model(bh, bt, mh, mt, bkg, **model_kwargs))
    e = batch["edge_indices"]
    heads, tails, labels = (e[x].to(device, torch.int64) for x in ("head", "tail", "label"))
    plan = ops.triple_plan(labels, heads, tails, int(model.decoder.out_features), mh.shape[0], mt.shape[0])
    return torch.sigmoid(model.score_triples(bh, bt, mh, mt, bkg, plan, **model_kwargs))


@torch.no_grad()
def make_predictions(ckpt_or_checkpoint_dir, batch: dict, eval_type: str, finetune_mode: str, device, force_ori_modalities: bool = False,
                     return_all_pairwise: bool = False, **model_kwargs) -> torch.Tensor:
    """predict.py:make_predictions -> sigmoid probabilities on the CPU: of the labelled triples of ``batch['edge_indices']`` in list
    order, or the dense [L, Nh, Nt] with ``return_all_pairwise``.  ``ckpt_or_checkpoint_dir`` is a ``.pt`` file, a directory prefix
    (``+ "best_model.pt"``) or a ``NovelDDIMultilabel``; a checkpoint is loaded with ``strict=False``, as in the reference.
    ``model_kwargs`` (an extension) go to the model's forward / ``score_triples`` (e.g. ``kg_filler``)."""
    if force_ori_modalities:
        raise NotImplementedError("make_predictions: force_ori_modalities is not implemented on the HIP path")
    model = _model(ckpt_or_checkpoint_dir, device)
    return _scores(model, batch, eval_type, finetune_mode, device, return_all_pairwise, **model_kwargs).cpu()


@torch.no_grad()
def get_drug_specific_scores(checkpoint_dir, batch: dict, eval_type: str, finetune_mode: str, device, mode: str = "test_between",
                             force_ori_modalities: bool = False, **model_kwargs):
    """predict.py:get_drug_specific_scores -> ``(all_metrics, drugs_of_interest)``: ``all_metrics`` maps the metric names of
    get_metrics (k = 50) to one np.float64 per drug of interest; ``drugs_of_interest`` is ``batch['head']['drugs']``
    (``test_between``) or ``batch['tail']['drugs']`` at the sorted tail indices of the positives (``test_between_train``).
    The probabilities stay on the device between the forward and the metrics.  Raises ValueError where the reference fails (see
    ``metrics.drug_specific_metrics``) and NotImplementedError for other modes and ``force_ori_modalities``."""
    if force_ori_modalities:
        raise NotImplementedError("get_drug_specific_scores: force_ori_modalities is not implemented on the HIP path")
    if mode not in MT._DRUG_MODES:
        raise NotImplementedError(f"get_drug_specific_scores: mode must be one of {MT._DRUG_MODES}, got {mode!r}")
    device = torch.device(device)
    model = _model(checkpoint_dir, device)
    pred = _scores(model, batch, eval_type, finetune_mode, device, False, **model_kwargs)
    e = batch["edge_indices"]
    heads, tails, labels, pos_neg = (e[x].to(device) for x in ("head", "tail", "label", "pos_neg"))
    n_head = int(batch["head"]["drugs"].shape[0])
    metrics, owners = MT.drug_specific_metrics(pred, heads, tails, labels, pos_neg, n_head, mode)
    side = batch["head"] if mode == "test_between" else batch["tail"]
    drugs = side["drugs"].cpu()
    return metrics, (drugs if mode == "test_between" else drugs[torch.from_numpy(owners)])
