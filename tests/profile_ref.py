"""Dense reference of the per-pair outcome profile (mdg_bilinear_profile), shared by tests/test_profile_cpu.py and
tests/test_profile_gpu.py: count, best and margin over a materialised score tensor [L, nh, nt] on any device."""
import torch

from bincount_ref import eligible_mask


def dense_profile(dense: torch.Tensor, thr: torch.Tensor, scale=None, eligible: str = "all"):
    """-> (count int32, best int32, margin fp32), each [nh, nt].  count[i,j] = #{l : dense[l,i,j] >= thr[l]}; u_l = (dense[l] -
    thr[l]) * scale[l], a subtract and then a multiply, each rounded to fp32; margin = max_l u_l with NaN never taking part and
    -inf where nothing exceeds -inf; best = the LOWEST l with u_l == margin (built with where / min: the tie order of argmax is
    unspecified), -1 where margin is -inf.  Ineligible pairs: 0 / -1 / -inf."""
    L, nh, nt = dense.shape
    dev = dense.device
    ninf = torch.tensor(float("-inf"), device=dev)
    elig = eligible_mask(nh, nt, eligible, dev)
    if L == 0:
        count = torch.zeros((nh, nt), dtype=torch.int32, device=dev)
        return count, torch.full_like(count, -1), torch.full((nh, nt), float("-inf"), device=dev)
    t3 = thr.to(dev)[:, None, None]
    count = (dense >= t3).sum(0).to(torch.int32)
    u = dense - t3
    if scale is not None:
        u = u * scale.to(dev)[:, None, None]
    u = torch.where(torch.isnan(u), ninf, u)
    margin = u.max(0).values
    ls = torch.arange(L, device=dev)[:, None, None]
    best = torch.where((u == margin[None]) & (margin[None] > ninf), ls, L).min(0).values
    best = torch.where(best == L, -1, best).to(torch.int32)
    count = torch.where(elig, count, 0)
    best = torch.where(elig, best, -1)
    margin = torch.where(elig, margin, ninf)
    return count, best, margin


def loop_profile(dense: torch.Tensor, thr: torch.Tensor, scale=None, eligible: str = "all"):
    """The same by a plain Python loop in the order the kernel walks: ascending l, moving only on u > margin."""
    L, nh, nt = dense.shape
    elig = eligible_mask(nh, nt, eligible)
    count = torch.zeros((nh, nt), dtype=torch.int32)
    best = torch.full((nh, nt), -1, dtype=torch.int32)
    margin = torch.full((nh, nt), float("-inf"))
    for i in range(nh):
        for j in range(nt):
            if not bool(elig[i, j]):
                continue
            for l in range(L):
                x = dense[l, i, j]
                if bool(x >= thr[l]):
                    count[i, j] += 1
                u = x - thr[l]
                if scale is not None:
                    u = u * scale[l]
                if bool(u > margin[i, j]):
                    margin[i, j] = u
                    best[i, j] = l
    return count, best, margin


def same(a, b) -> bool:
    """Two (count, best, margin) triples are equal, the margins bit for bit."""
    return torch.equal(a[0], b[0]) and torch.equal(a[1].to(torch.int64), b[1].to(torch.int64)) and \
        torch.equal(a[2].contiguous().view(torch.int32), b[2].contiguous().view(torch.int32))
