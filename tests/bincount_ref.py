"""Brute-force references shared by tests/test_bincount_cpu.py and tests/test_bincount_gpu.py: counts between edges, counts
below a query and tie groups, all over a materialised dense score tensor (any device)."""
import torch


def eligible_mask(nh: int, nt: int, eligible: str, device="cpu") -> torch.Tensor:
    """bool [nh, nt]: the entries mdg_topk_eligible's mode keeps."""
    i = torch.arange(nh, device=device)[:, None]
    j = torch.arange(nt, device=device)[None, :]
    if eligible == "all":
        return torch.ones((nh, nt), dtype=torch.bool, device=device)
    if eligible == "not_self":
        return i != j
    if eligible == "lower":
        return j < i
    raise ValueError(eligible)


def eligible_scores(dense: torch.Tensor, eligible: str) -> torch.Tensor:
    """[L, M]: the eligible entries of dense [L, nh, nt], row-major."""
    m = eligible_mask(dense.shape[1], dense.shape[2], eligible, dense.device)
    return dense[:, m]


def brute_counts(dense: torch.Tensor, edges: torch.Tensor, eligible: str) -> torch.Tensor:
    """int64 [L, B+1]: torch.bucketize(right=True) + bincount of the eligible entries of every outcome."""
    vals = eligible_scores(dense, eligible)
    B = edges.shape[1]
    out = []
    for l in range(dense.shape[0]):
        b = torch.bucketize(vals[l].contiguous(), edges[l].contiguous(), right=True)
        out.append(torch.bincount(b, minlength=B + 1))
    return torch.stack(out)


def brute_less(vals: torch.Tensor, queries: torch.Tensor, shift: float = 0.0) -> torch.Tensor:
    """int64 [L, Q]: for every query the number of vals [L, M] strictly below ``query + shift`` (compared in float64)."""
    sv = torch.sort(vals.double(), dim=1).values
    return torch.searchsorted(sv, queries.double() + shift, right=False)


def is_unique(vals: torch.Tensor, queries: torch.Tensor) -> torch.Tensor:
    """bool [L, Q]: the query's value occurs at most once among vals [L, M] of its outcome."""
    sv = torch.sort(vals, dim=1).values.contiguous()
    q = queries.contiguous()
    return (torch.searchsorted(sv, q, right=True) - torch.searchsorted(sv, q, right=False)) <= 1


def inputs(nh: int, nt: int, L: int, seed: int = 0):
    """Head / tail embeddings and weights as tests/test_topk_gpu.py builds them: tail rows 5, 9 and nt - 2 are copies of row 3
    (exact ties); nh == nt is ONE drug set, with z_tail a separate copy of z_head, so that the dense head takes the general
    sweep (whose scores the counting sweep reproduces bit for bit) and not the symmetric one."""
    def rand(shape, s, scale=1.0):
        return torch.randn(shape, generator=torch.Generator().manual_seed(s)) * scale
    w = rand((L, 128, 128), seed + 3, 1 / 128 ** 0.5)
    zt = rand((nt, 128), seed + 2)
    for dup in (5, 9, nt - 2):
        if 3 < dup < nt:
            zt[dup] = zt[3]
    zh = zt.clone() if nh == nt else rand((nh, 128), seed + 1)
    return zh, zt, w
