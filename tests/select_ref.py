"""Brute-force references shared by tests/test_select_cpu.py and tests/test_select_gpu.py: the CSR of every eligible entry of a
materialised dense score tensor at or above a per-outcome cut (any device)."""
import torch

from bincount_ref import eligible_mask


def dense_mask(dense: torch.Tensor, thr: torch.Tensor, eligible: str) -> torch.Tensor:
    """bool [L, nh, nt]: (dense[l] >= thr[l]) & eligible."""
    return (dense >= thr.to(dense.device)[:, None, None]) & eligible_mask(dense.shape[1], dense.shape[2], eligible, dense.device)[None]


def csr_of_mask(dense: torch.Tensor, mask: torch.Tensor):
    """(row_counts int32 [L, nh], row_ptr int64 [L*nh + 1], cols int32 [T], vals fp32 [T]) of a bool mask over dense [L, nh, nt], in
    torch.nonzero's order: rows l * nh + i ascending, columns ascending within a row."""
    L, nh, _ = dense.shape
    counts = mask.sum(2)
    row_ptr = torch.zeros(L * nh + 1, dtype=torch.int64, device=dense.device)
    row_ptr[1:] = torch.cumsum(counts.reshape(-1), 0)
    nz = mask.nonzero()
    return counts.to(torch.int32), row_ptr, nz[:, 2].to(torch.int32), dense[nz[:, 0], nz[:, 1], nz[:, 2]]


def dense_csr(dense: torch.Tensor, thr: torch.Tensor, eligible: str):
    """csr_of_mask of (dense[l] >= thr[l]) & eligible."""
    return csr_of_mask(dense, dense_mask(dense, thr, eligible))
