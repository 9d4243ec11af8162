"""Dense CPU reference of the streaming per-pair top-k over outcomes (mdg_outcome_topk_update / ops.outcome_topk), shared by
tests/test_outcome_topk_cpu.py and tests/test_outcome_topk_gpu.py: the whole tensor at once, sorted with torch."""
import torch

INF = float("inf")


def outcome_topk_ref(x, k, labels=None, label_base=0, shift=None, scale=None, largest=True, eligible="all"):
    """(vals fp32 [k,Nh,Nt], idx int32 [k,Nh,Nt]) of x [L,Nh,Nt] (any float dtype, widened exactly) on the CPU:
    1. shift and scale applied in fp32 as two operations; 2. NaN values, sentinel-valued entries and planes with a negative label are
    absent; 3. planes ordered by label ascending; 4. a stable sort along dim 0 (descending, or ascending for largest=False);
    5. the first k, padded with the sentinels (-inf or +inf, -1).  eligible="lower": only entries with i > j, sentinels elsewhere."""
    v = x.detach().cpu().float().clone()
    L, nh, nt = v.shape
    if shift is not None:
        v = v - shift.detach().cpu().float()[:, None, None]
    if scale is not None:
        v = v * scale.detach().cpu().float()[:, None, None]
    lab = torch.arange(label_base, label_base + L) if labels is None else torch.as_tensor(labels).detach().cpu().long()
    sentinel = -INF if largest else INF
    absent = torch.isnan(v) | (v == sentinel) | (lab < 0)[:, None, None]
    order = torch.sort(lab, stable=True).indices
    v, absent, lab = v[order], absent[order], lab[order]
    v = torch.where(absent, torch.full_like(v, sentinel), v)
    ids = torch.where(absent, torch.full((1, 1, 1), -1, dtype=torch.long), lab[:, None, None].expand(L, nh, nt))
    if L < k:
        v = torch.cat([v, torch.full((k - L, nh, nt), sentinel)], 0)
        ids = torch.cat([ids, torch.full((k - L, nh, nt), -1, dtype=torch.long)], 0)
    pos = torch.sort(v, dim=0, descending=largest, stable=True).indices[:k]
    vals, idx = v.gather(0, pos), ids.gather(0, pos).to(torch.int32)
    if eligible == "lower":
        out = torch.arange(nt)[None, :] >= torch.arange(nh)[:, None]
        vals = vals.masked_fill(out[None], sentinel)
        idx = idx.masked_fill(out[None], -1)
    return vals, idx


def same_state(got, ref) -> bool:
    """torch.equal on vals and on idx (a GPU state against a CPU reference state)."""
    return torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])
