"""A device-resident drug store and on-device batch collation.

The reference collates every pretraining batch on the host: ``DrugCLCollator.__call__`` (madrigal/data/data.py:1479-1501)
indexes ``all_molecules``, ``tabular_mod_stores['cv']`` and the 16 ``tx_store_dict`` entries with the batch's drug ids, for
every iteration of pretrain.py and for every subset evaluate_pt looks at.  Here the modalities of every drug live on the GPU
once (:class:`DrugStore`, plain torch ops, built at start-up) and :class:`DeviceCollator` cuts a batch out of them with four
kernel launches (csrc/collate.hip), the molecule batch arriving with its aggregation plan (``graph_plans.molecule_plan``)
already attached: nothing is sorted, counted or scanned per batch.

The one visible difference from ``all_molecules[ids]``: inside a molecule the edges come in the store's order, stably sorted
by destination atom -- the order ``molecule_plan`` would sort them to -- instead of the order of the source file.  Atom order,
edge multiset, features and weights are the same, and so is every result of the structure encoder.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .data import BOND_DIM, CELL_LINES, CV_DIM, MOL_DIM, NUM_MODALITIES, TX_DIM, MoleculeBatch, as_molecule_batch

AUG_DIM = 20          # 18 bond features, the ones column, zero padding to a multiple of 4 (graph_plans.molecule_plan)


class CollatedMolecules(MoleculeBatch):
    """The molecule batch of a :class:`DeviceCollator` call.  ``to`` / ``cuda`` to the device it lives on return the object
    itself (and with it the attached plan) instead of a copy: ``evaluate._to`` moves whatever a collator hands over."""

    def to(self, device):
        dev = torch.device(device)
        here = self.node_feature.device
        if dev.type == here.type and (dev.index is None or dev.index == here.index):
            return self
        return super().to(device)


def _is_int(x) -> bool:
    """A Python / numpy integer or a 0-dim integer tensor (not a bool)."""
    if isinstance(x, torch.Tensor):
        return x.dim() == 0 and x.dtype != torch.bool and not x.is_floating_point() and not x.is_complex()
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def _ptr_from_counts(counts: torch.Tensor) -> torch.Tensor:
    ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, out=ptr[1:])
    return ptr


class DrugStore:
    """Every drug's modalities as plain tensors on one device.

    ``drugs [M]`` int64 (unique), ``id2row [max id + 1]`` (-1 = absent).  Molecules packed: ``atom_ptr edge_ptr [M+1]``,
    ``node_feature [A,67]``, ``edge_list [E,3]`` (store-wide atom numbers), ``edge_feature [E,18]``, ``edge_weight [E]``,
    ``edge_feat_aug [E,20]`` (the augmented rows of ``molecule_plan``), ``rowptr [A+1]`` (CSR over destination atoms); the
    edges of each molecule stably sorted by destination atom.  ``cv [M,559]``, ``sigs [16,M,978]``, ``dosages [16,M]`` (cell
    lines in ``data.CELL_LINES`` order), ``masks [M,19]`` bool or None, ``kg``: the dict ``{'data','drug_index_map'}`` as given.
    """

    def __init__(self, **fields):
        self.__dict__.update(fields)

    # ------------------------------------------------------------------------------------------------------------ building
    @classmethod
    def from_batch(cls, batch: dict, batch_kg: dict) -> "DrugStore":
        """From one side of the collator's output dict (``'drugs' 'strs' 'cv' 'tx' 'masks'``) and ``batch_kg``: row r of the
        batch belongs to drug id ``batch['drugs'][r]``."""
        return cls.from_stores(batch["strs"], batch_kg, batch["cv"], batch["tx"], masks=batch.get("masks"), drugs=batch["drugs"])

    @classmethod
    def from_stores(cls, molecules, kg_dict, cv, tx_store_dict, masks=None, drugs=None) -> "DrugStore":
        """From the reference collator's attributes (data.py:1426-1477): ``all_molecules`` (anything ``data.as_molecule_batch``
        reads), the KG dict, ``tabular_mod_stores['cv']`` [M,559] and ``tx_store_dict`` {cell line: {'sigs' [M,978], 'dosages'
        [M], ...}}.  ``drugs``: the id of every row (default 0..M-1).  The tensors stay on the device of ``molecules``."""
        mols = as_molecule_batch(molecules)
        dev = mols.node_feature.device
        M = int(mols.batch_size)
        drugs = torch.arange(M, dtype=torch.int64, device=dev) if drugs is None else torch.as_tensor(drugs).to(dev).long().reshape(-1)
        if drugs.numel() != M:
            raise ValueError(f"DrugStore: {drugs.numel()} drug ids for {M} molecules")
        if M == 0:
            raise ValueError("DrugStore: no drugs")
        if int(drugs.min()) < 0 or torch.unique(drugs).numel() != M:
            raise ValueError("DrugStore: drug ids must be unique and non-negative")
        id2row = torch.full((int(drugs.max()) + 1,), -1, dtype=torch.int64, device=dev)
        id2row[drugs] = torch.arange(M, dtype=torch.int64, device=dev)

        nf = mols.node_feature.float().contiguous()
        n2g = mols.node2graph.long()
        A = int(nf.shape[0])
        if nf.dim() != 2 or nf.shape[1] != MOL_DIM:
            raise ValueError(f"DrugStore: node_feature must be [A,{MOL_DIM}], got {tuple(nf.shape)}")
        if n2g.numel() != A or (A and (int(n2g.min()) < 0 or int(n2g.max()) >= M)) or (A > 1 and not bool(torch.all(n2g[1:] >= n2g[:-1]))):
            raise ValueError("DrugStore: node2graph must be non-decreasing with values in [0, batch_size) (packed graphs)")
        atom_ptr = _ptr_from_counts(torch.bincount(n2g, minlength=M))
        el = mols.edge_list.long()
        ef = mols.edge_feature.float()
        ew = mols.edge_weight.float()
        E = int(el.shape[0])
        if el.shape[1:] != (3,) or ef.shape != (E, BOND_DIM) or ew.shape != (E,):
            raise ValueError(f"DrugStore: edge_list [E,3], edge_feature [E,{BOND_DIM}] and edge_weight [E] expected, got "
                             f"{tuple(el.shape)}, {tuple(ef.shape)}, {tuple(ew.shape)}")
        if E and (int(el[:, :2].min()) < 0 or int(el[:, :2].max()) >= A):
            raise ValueError("DrugStore: edge_list names an atom outside the batch")
        if E and not bool(torch.all(n2g[el[:, 0]] == n2g[el[:, 1]])):
            raise ValueError("DrugStore: an edge joins atoms of two molecules")
        # atoms are packed molecule by molecule, so ONE stable sort by destination atom groups the edges by molecule and,
        # inside a molecule, by destination, equal destinations in their original order
        order = torch.argsort(el[:, 1], stable=True)
        el, ef, ew = el[order].contiguous(), ef[order].contiguous(), ew[order].contiguous()
        edge_ptr = _ptr_from_counts(torch.bincount(n2g[el[:, 1]], minlength=M))
        rowptr = _ptr_from_counts(torch.bincount(el[:, 1], minlength=A))
        aug = torch.cat([ef, torch.ones(E, 1, device=dev), torch.zeros(E, AUG_DIM - BOND_DIM - 1, device=dev)], dim=1).contiguous()

        cv = torch.as_tensor(cv).to(dev).float().contiguous()
        if cv.shape != (M, CV_DIM):
            raise ValueError(f"DrugStore: cv must be [{M},{CV_DIM}], got {tuple(cv.shape)}")
        missing = [c for c in CELL_LINES if c not in tx_store_dict]
        if missing:
            raise ValueError(f"DrugStore: tx_store_dict lacks the cell lines {missing}")
        sigs = torch.stack([torch.as_tensor(tx_store_dict[c]["sigs"]).to(dev).float() for c in CELL_LINES]).contiguous()
        dosages = torch.stack([torch.as_tensor(tx_store_dict[c]["dosages"]).to(dev).float() for c in CELL_LINES]).contiguous()
        if sigs.shape != (len(CELL_LINES), M, TX_DIM) or dosages.shape != (len(CELL_LINES), M):
            raise ValueError(f"DrugStore: tx sigs must be [{M},{TX_DIM}] and dosages [{M}] per cell line, got {tuple(sigs.shape[1:])} "
                             f"and {tuple(dosages.shape[1:])}")
        if masks is not None:
            masks = torch.as_tensor(masks).to(dev).bool().contiguous()
            if masks.shape != (M, NUM_MODALITIES):
                raise ValueError(f"DrugStore: masks must be [{M},{NUM_MODALITIES}], got {tuple(masks.shape)}")
        return cls(drugs=drugs, id2row=id2row, n_drugs=M, atom_ptr=atom_ptr, edge_ptr=edge_ptr, node_feature=nf, edge_list=el,
                   edge_feature=ef, edge_weight=ew, edge_feat_aug=aug, rowptr=rowptr, unit_weights=bool(torch.all(ew == 1.0)),
                   cv=cv, sigs=sigs, dosages=dosages, masks=masks, kg=kg_dict)

    _TENSORS = ("drugs", "id2row", "atom_ptr", "edge_ptr", "node_feature", "edge_list", "edge_feature", "edge_weight", "edge_feat_aug",
                "rowptr", "cv", "sigs", "dosages", "masks")

    @property
    def device(self):
        return self.node_feature.device

    def to(self, device) -> "DrugStore":
        """The store on ``device`` (the KG dict moves with it: ``data.to(device)``, ``drug_index_map.to(device)``)."""
        fields = dict(self.__dict__)
        for k in self._TENSORS:
            if fields[k] is not None:
                fields[k] = fields[k].to(device)
        kg = self.kg
        if kg is not None:
            fields["kg"] = {k: (v.to(device) if hasattr(v, "to") and not isinstance(v, np.ndarray) else v) for k, v in kg.items()}
        return DrugStore(**fields)

    def cuda(self) -> "DrugStore":
        return self.to("cuda")

    # ---------------------------------------------------------------------------------------------------------- collation
    def ids_of(self, batch) -> torch.Tensor:
        """The drug ids of a collator argument as a 1-D int64 tensor on the store's device: ``[tensor]``, ``[ndarray]``, a list
        of ints, a list of 1-tuples (what a DataLoader hands ``DrugCLCollator``, data.py:1480-1489) or a bare tensor / array."""
        if isinstance(batch, (torch.Tensor, np.ndarray)):
            ids = batch
        elif isinstance(batch, (list, tuple)):
            if len(batch) == 0:
                raise ValueError("collate: empty id list")
            first = batch[0]
            if (isinstance(first, torch.Tensor) and first.dim() > 0) or (isinstance(first, np.ndarray) and first.ndim > 0):
                if len(batch) != 1:
                    raise ValueError(f"collate: expected [ids], got a list of {len(batch)} arrays")
                ids = first
            elif isinstance(first, (tuple, list)):
                if any(len(x) != 1 for x in batch):
                    raise ValueError("collate: a list of tuples must hold 1-tuples (one drug id each)")
                ids = [x[0] for x in batch]
            else:
                ids = list(batch)
        else:
            raise ValueError(f"collate: cannot read drug ids from {type(batch).__name__}")
        if isinstance(ids, list):
            if not all(_is_int(x) for x in ids):
                raise ValueError("collate: drug ids must be integers")
            ids = torch.tensor([int(x) for x in ids], dtype=torch.int64)
        elif isinstance(ids, np.ndarray):
            if not np.issubdtype(ids.dtype, np.integer):
                raise ValueError(f"collate: drug ids must be integers, got dtype {ids.dtype}")
            ids = torch.from_numpy(np.ascontiguousarray(ids).astype(np.int64, copy=False))
        if ids.dtype in (torch.bool,) or ids.is_floating_point() or ids.is_complex():
            raise ValueError(f"collate: drug ids must be integers, got dtype {ids.dtype}")
        if ids.dim() != 1:
            raise ValueError(f"collate: drug ids must be one-dimensional, got shape {tuple(ids.shape)}")
        if ids.numel() == 0:
            raise ValueError("collate: empty id list")
        return ids.to(device=self.device, dtype=torch.int64).contiguous()

    def collate(self, batch) -> dict:
        """The drugs ``batch`` names (any order, duplicates allowed) as fresh tensors: ``{'ids' 'rows' 'strs' 'cv' 'sigs'
        'dosages'}`` with ``strs`` a packed molecule batch carrying its plan, ``sigs [16,B,978]``, ``dosages [16,B]``.
        Four launches whatever B is -- two for the offsets, one for the tabular rows, one for the molecules -- and one
        device-to-host read (atoms, edges, status) between the third and the fourth."""
        if self.device.type != "cuda":
            raise ValueError(f"collate: the store must live on the GPU (it is on {self.device}); the HIP path has no CPU fallback")
        ids = self.ids_of(batch)
        B = int(ids.numel())
        rows, out_atom_ptr, out_edge_ptr, totals = ops.collate_offsets(ids, self.id2row, self.atom_ptr, self.edge_ptr)
        sigs, dosages, cv = ops.collate_rows([self.sigs, self.dosages.unsqueeze(2), self.cv.unsqueeze(0)], rows)
        A, E, bad, first_bad = totals.tolist()                   # the one device-to-host read (it also orders the launches above)
        if bad:
            raise ValueError(f"collate: {bad} of {B} drug ids are not in the store (the first: id {int(ids[first_bad])} at position {first_bad})")
        m = ops.collate_molecules(rows, out_atom_ptr, out_edge_ptr, A, E, self.atom_ptr, self.edge_ptr, self.node_feature, self.edge_list,
                                  self.edge_feature, self.edge_weight, self.edge_feat_aug, self.rowptr,
                                  want_w=not self.unit_weights and E > 0)      # a batch without edges: w None, as molecule_plan has it
        mols = CollatedMolecules(m["node_feature"], m["edge_list"], m["edge_feature"], m["node2graph"], B, m["edge_weight"])
        mols._mdg_plan = {"device": m["node_feature"].device, "rowptr": m["rowptr"], "col": m["col"], "w": m["w"],
                          "edge_feat_aug": m["edge_feat_aug"], "edge_feat_dim": BOND_DIM, "graph_rowptr": out_atom_ptr, "n_graphs": B}
        return {"ids": ids, "rows": rows, "strs": mols, "cv": cv[0], "sigs": sigs, "dosages": dosages[:, :, 0]}

    @staticmethod
    def _tx(c: dict) -> dict:
        B = int(c["ids"].numel())
        return {name: {"sigs": c["sigs"][k], "drugs": c["ids"], "dosages": c["dosages"][k], "cell_lines": np.full(B, name)}
                for k, name in enumerate(CELL_LINES)}

    def batch(self, ids) -> dict:
        """The finetune-side batch dict ``{'drugs','strs','cv','tx','masks'}`` of a subset of the store's drugs, for
        ``pipeline.generate_embeddings`` / ``make_predictions``; ``masks = store.masks[rows]``."""
        if self.masks is None:
            raise ValueError("DrugStore.batch: the store was built without masks")
        c = self.collate(ids)
        return {"drugs": c["ids"], "strs": c["strs"], "cv": c["cv"], "tx": self._tx(c), "masks": self.masks.index_select(0, c["rows"])}


class DeviceCollator:
    """Callable like ``DrugCLCollator`` (data.py:1479-1501): ``collator([ids]) -> (ids, (mols, kg_dict, cv, tx))``.

    ``ids`` int64 on the device; ``mols`` a packed batch with ``batch_size = B`` whose atoms are those of ids[0], ids[1], ...
    and whose ``_mdg_plan`` is attached (``w`` None when every weight of the STORE is 1); ``kg_dict`` the store's own dict,
    the same object on every call (the reference clones the whole KG when ``kg_sampling_num_neighbors`` is None; the HGT plan
    caches are keyed on the object); ``cv [B,559]``; ``tx[c] = {'sigs' [B,978] (a slice of one [16,B,978] buffer), 'drugs'
    (ids), 'dosages' [B], 'cell_lines' (numpy array of B names)}``.  Every call returns new tensors and new containers."""

    def __init__(self, store: DrugStore):
        if not isinstance(store, DrugStore):
            raise ValueError("DeviceCollator: expected a DrugStore")
        self.store = store

    def __call__(self, batch):
        c = self.store.collate(batch)
        return c["ids"], (c["strs"], self.store.kg, c["cv"], DrugStore._tx(c))
