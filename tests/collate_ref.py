"""Host checker of the on-device collation (madrigal_amd/collate.py): a per-drug gather from the ORIGINAL batch, whose edges
are in generation order (not sorted by destination), the way ``all_molecules[ids]`` of the reference gathers
(madrigal/data/data.py:1479-1501).  Plain torch on CPU tensors; nothing of madrigal_amd.collate is used."""
import numpy as np
import torch

from madrigal_amd import data as D


def _one_hot(rng, n, blocks):
    out = np.zeros((n, sum(blocks)), dtype=np.float32)
    off = 0
    for b in blocks:
        out[np.arange(n), off + rng.integers(0, b, size=n)] = 1.0
        off += b
    return out


def hand_molecule(n_atoms, seed):
    """One molecule made by hand: a chain of ``n_atoms`` atoms plus a few ring closures, every bond in both directions (all
    forward directions first, so the edges are NOT sorted by destination); a single atom has no edges."""
    rng = np.random.default_rng([seed, 707])
    u = np.arange(1, n_atoms, dtype=np.int64)
    v = u - 1
    if n_atoms > 8:
        ru = rng.integers(0, n_atoms, size=n_atoms // 12)
        rv = (ru + 5) % n_atoms
        u, v = np.concatenate([u, ru]), np.concatenate([v, rv])
    f = _one_hot(rng, u.shape[0], (4, 3, 6, 2, 3))
    src, dst, ef = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([f, f])
    el = np.stack([src, dst, ef[:, :4].argmax(1).astype(np.int64) if ef.shape[0] else np.zeros(0, np.int64)], 1).astype(np.int64)
    nf = _one_hot(rng, n_atoms, (18, 7, 7, 8, 7, 6, 7, 2, 5))
    return torch.from_numpy(nf), torch.from_numpy(el), torch.from_numpy(ef.reshape(-1, 18))


def make_store_batch(seed, weighted=False, n=64):
    """``make_batch(64, seed, kg_nodes=600, kg_edges=6000)`` with two molecules appended by hand: drug 64 has one atom and no
    edge, drug 65 has 300 atoms.  The two own the structure modality only (their cv / tx rows are still random numbers, so a
    gather of them is checked).  ``weighted``: non-unit edge weights on every molecule.  -> (batch, batch_kg), CPU."""
    masks = D.make_masks(n, seed, p_kg=0.7, p_cv=0.7, p_tx=0.5)
    batch, bkg = D.make_batch(n, seed, kg_nodes=600, kg_edges=6000, masks=masks)
    rng = np.random.default_rng([seed, 808])
    m = batch["strs"]
    nfs, els, efs, n2g, base = [m.node_feature], [m.edge_list], [m.edge_feature], [m.node2graph], m.num_node
    for g, atoms in ((n, 1), (n + 1, 300)):
        nf, el, ef = hand_molecule(atoms, seed + g)
        el = el.clone()
        el[:, :2] += base
        nfs.append(nf); els.append(el); efs.append(ef)
        n2g.append(torch.full((atoms,), g, dtype=torch.int64))
        base += atoms
    el = torch.cat(els)
    ew = torch.from_numpy((0.5 + rng.random(el.shape[0])).astype(np.float32)) if weighted else None
    mols = D.MoleculeBatch(torch.cat(nfs), el, torch.cat(efs), torch.cat(n2g), n + 2, ew)
    extra = torch.ones(2, D.NUM_MODALITIES, dtype=torch.bool)
    extra[:, 0] = False
    tx = {}
    for c, v in batch["tx"].items():
        tx[c] = {"sigs": torch.cat([v["sigs"], torch.from_numpy(rng.standard_normal((2, D.TX_DIM)).astype(np.float32))]),
                 "drugs": torch.arange(n + 2, dtype=torch.int64),
                 "dosages": torch.cat([v["dosages"], torch.from_numpy(rng.uniform(0, 10, size=2).astype(np.float32))]),
                 "cell_lines": np.array([c] * (n + 2), dtype=np.str_)}
    out = {"drugs": torch.arange(n + 2, dtype=torch.int64), "strs": mols,
           "cv": torch.cat([batch["cv"], torch.from_numpy(rng.standard_normal((2, D.CV_DIM)).astype(np.float32))]),
           "tx": tx, "masks": torch.cat([masks, extra])}
    return out, bkg


class HostCollator:
    """collator([ids]) -> (ids, (mols, kg, cv, tx)): rows of one batch gathered drug by drug (``ids`` index rows: the batches
    here number their drugs 0..n-1).  Molecule r keeps its atoms and, in their original order, the edges that end in them."""

    def __init__(self, batch, kg):
        self.b, self.kg = batch, kg
        m = batch["strs"]
        self.pieces = []
        for r in range(m.batch_size):
            atoms = torch.nonzero(m.node2graph == r).flatten()
            a0, a1 = (int(atoms[0]), int(atoms[-1]) + 1) if atoms.numel() else (0, 0)
            keep = (m.edge_list[:, 1] >= a0) & (m.edge_list[:, 1] < a1)
            el = m.edge_list[keep].clone()
            el[:, :2] -= a0
            self.pieces.append((m.node_feature[a0:a1], el, m.edge_feature[keep], m.edge_weight[keep]))

    def molecules(self, ids):
        nf, el, ef, ew, n2g, base = [], [], [], [], [], 0
        for g, r in enumerate(ids.tolist()):
            p = self.pieces[r]
            e = p[1].clone()
            e[:, :2] += base
            nf.append(p[0]); el.append(e); ef.append(p[2]); ew.append(p[3])
            n2g.append(torch.full((p[0].shape[0],), g, dtype=torch.int64))
            base += p[0].shape[0]
        return D.MoleculeBatch(torch.cat(nf), torch.cat(el), torch.cat(ef), torch.cat(n2g), len(ids), torch.cat(ew))

    def __call__(self, arg):
        ids = torch.as_tensor(np.asarray(arg[0]), dtype=torch.int64)
        b = self.b
        tx = {c: {"sigs": v["sigs"][ids], "drugs": v["drugs"][ids], "dosages": v["dosages"][ids],
                  "cell_lines": v["cell_lines"][ids.numpy()]} for c, v in b["tx"].items()}
        return ids, (self.molecules(ids), self.kg, b["cv"][ids], tx)


def sorted_by_destination(mols):
    """(edge_list, edge_feature, edge_weight) of a packed batch permuted by the stable argsort of the destinations."""
    order = torch.argsort(mols.edge_list[:, 1], stable=True)
    return mols.edge_list[order], mols.edge_feature[order], mols.edge_weight[order]


PLAN_KEYS = ("device", "rowptr", "col", "w", "edge_feat_aug", "edge_feat_dim", "graph_rowptr", "n_graphs")


def assert_plans_equal(got, want):
    """Field by field: the same keys, equal tensors (dtype, shape, values), equal scalars; ``w`` None on both sides or on neither."""
    assert set(got) == set(want) == set(PLAN_KEYS), (sorted(got), sorted(want))
    for k in PLAN_KEYS:
        g, w = got[k], want[k]
        if isinstance(w, torch.Tensor):
            assert isinstance(g, torch.Tensor) and g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (k, g, w)
            assert g.is_contiguous(), k
            assert torch.equal(g, w), k
        else:
            assert g == w and type(g) is type(w), (k, g, w)
