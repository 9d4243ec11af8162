"""plan["q_slot"] of TransformerFusion.live_token_plan / merged_live_plan: the inverse of key_rows over the live rows (no GPU)."""
import pytest
import torch


def _fusion(agg, nb):
    import madrigal_amd.models as M
    return M.TransformerFusion(128, nb, 2, 2, 32, 64, 0.0, "gelu", True, False, agg)


def _mask(m, n, seed):
    from madrigal_amd.data import NUM_MODALITIES, NUM_NON_TX_MODALITIES
    nb, has_cls = m.num_tx_bottlenecks, 1 if m.transformer_agg == "cls" else 0
    g = torch.Generator().manual_seed(seed)
    kpm = torch.rand(n, has_cls + NUM_MODALITIES + nb, generator=g) < 0.6
    kpm[:, :has_cls] = False
    kpm[:, has_cls + NUM_NON_TX_MODALITIES:has_cls + NUM_NON_TX_MODALITIES + nb] = False
    return kpm


def _check(plan):
    key_rows, q_slot, R = plan["key_rows"], plan["q_slot"], plan["R"]
    assert q_slot.dtype == torch.int32 and q_slot.shape == (R,) and q_slot.is_contiguous()
    assert bool((key_rows[1:] > key_rows[:-1]).all())                      # ascending: slot i <-> key_rows[i]
    assert torch.equal(q_slot[key_rows].long(), torch.arange(key_rows.numel()))
    rest = torch.ones(R, dtype=torch.bool)
    rest[key_rows] = False
    assert bool((q_slot[rest] == -1).all()) and int((q_slot >= 0).sum()) == key_rows.numel()


@pytest.mark.parametrize("agg,nb", [("x-attn", 4), ("x-attn", 2), ("cls", 2)])
def test_q_slot_is_the_inverse_of_key_rows(agg, nb):
    m = _fusion(agg, nb)
    a, b = m.live_token_plan(_mask(m, 37, 1), None), m.live_token_plan(_mask(m, 5, 2), None)
    _check(a)
    _check(b)
    merged = m.merged_live_plan(a, b)
    _check(merged)
    assert torch.equal(merged["q_slot"][:a["R"]], a["q_slot"])
    tail, shifted = merged["q_slot"][a["R"]:], b["q_slot"] + a["key_rows"].numel()
    assert torch.equal(tail, torch.where(b["q_slot"] >= 0, shifted, torch.full_like(shifted, -1)))


def test_a_plan_without_kept_rows_has_no_q_slot():
    m = _fusion("mean", 2)
    assert "q_slot" not in m.live_token_plan(_mask(m, 9, 3), None)
