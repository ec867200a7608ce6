"""Python mirror of the reference's S4 class `infercnv` (R/inferCNV.R:37-47).

The class is the data model of the drop-in boundary: every step function takes
an object and returns an object, touching only `expr_data` (and, by recursion,
`hspike`), exactly like the R functions called from run()
(R/inferCNV_ops.R:771-1589).  Index vectors are 0-based here (R: 1-based).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np


@dataclass
class GeneOrder:
    """gene_order data.frame(chr, start, stop); `chr` kept as strings/codes."""
    chr: np.ndarray
    start: Optional[np.ndarray] = None
    stop: Optional[np.ndarray] = None


class DeviceMatrix:
    """A genes x cells matrix that lives where its tensor lives -- in HBM for a CUDA tensor -- in the slot `expr_data`
    (DESIGN K32).  It wraps a contiguous (C cells, G genes) tensor, which is byte for byte R's column-major genes x cells
    matrix (device.py), and reports R's shape: `.shape == (G, C)`.

    kind "expr":   float64 values.
    kind "states": uint8 HMM states, 255 = a cell no HMM touched (the state objects of hmm.py).

    Nothing converts it silently: `__array__` raises TypeError, so NumPy code that has not been taught the type fails
    loudly instead of pulling the matrix across PCIe.  `to_host()` is the one way out and `from_host()` the one way in;
    both are counted (`DeviceMatrix.stats()`).  CPU tensors are accepted: the class works without a GPU, and then "across
    PCIe" is a copy in host memory that is counted all the same."""

    KINDS = {"expr": "float64", "states": "uint8"}
    _stats = {"uploads": 0, "fetches": 0, "bytes_up": 0, "bytes_down": 0}

    def __init__(self, tensor, kind: str = "expr"):
        import torch
        if kind not in self.KINDS:
            raise ValueError(f"kind must be one of {sorted(self.KINDS)}, not {kind!r}")
        want = getattr(torch, self.KINDS[kind])
        if not (isinstance(tensor, torch.Tensor) and tensor.dim() == 2 and tensor.dtype == want and tensor.is_contiguous()):
            raise TypeError(f"a {kind!r} DeviceMatrix wraps a contiguous {want} tensor of shape (cells, genes)")
        self._t = tensor
        self.kind = kind

    # ---- what the object code reads ----------------------------------------
    @property
    def tensor(self):
        return self._t

    @property
    def shape(self):
        return (int(self._t.shape[1]), int(self._t.shape[0]))

    ndim = 2

    @property
    def size(self):
        return int(self._t.numel())

    @property
    def nbytes(self):
        return int(self._t.numel() * self._t.element_size())

    @property
    def device(self):
        return self._t.device

    def float_tensor(self):
        """The values as the host route's float64 matrix holds them, on the tensor's device: the tensor itself for "expr"; for
        "states" a float64 copy with -1 for the untouched cells (what plot_cnv and the proxy steps read)."""
        if self.kind == "expr":
            return self._t
        import torch
        out = self._t.to(torch.float64)
        out[self._t == 255] = -1.0
        return out

    def __repr__(self):
        return f"DeviceMatrix(kind={self.kind!r}, shape={self.shape}, device={str(self._t.device)!r})"

    def __array__(self, *args, **kwargs):
        raise TypeError("a DeviceMatrix does not convert to a NumPy array by itself: this code path has not been wired for "
                        "device-resident objects.  Call to_host() on the matrix (or on the InfercnvObject) to fetch it.")

    # ---- the two counted crossings -----------------------------------------
    @classmethod
    def from_host(cls, array, kind: str = "expr", device=None):
        """Upload the (G, C) host matrix an object holds.  States: float64 with -1 for untouched cells (hmm._states_obj)
        or uint8 with 255."""
        import torch
        a = np.asarray(array)
        if a.ndim != 2:
            raise ValueError("expected a genes x cells matrix")
        if kind == "states":
            if a.dtype != np.uint8:
                a = np.where(a < 0, 255, a).astype(np.uint8)
        else:
            a = a.astype(np.float64, copy=False)
        host = torch.from_numpy(np.ascontiguousarray(a.T))
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        t = host.to(device).clone() if torch.device(device).type == "cpu" else host.to(device)
        cls._stats["uploads"] += 1
        cls._stats["bytes_up"] += int(t.numel() * t.element_size())
        return cls(t, kind)

    def to_host(self):
        """The F-ordered (G, C) float64 array the host route holds in this slot; for states 255 becomes -1."""
        cls = type(self)
        cls._stats["fetches"] += 1
        cls._stats["bytes_down"] += self.nbytes
        a = self._t.cpu().numpy()                               # (C, G), C-contiguous
        if self.kind == "states":
            out = a.astype(np.float64)
            out[a == 255] = -1.0
            return out.T
        return (a.copy() if self._t.device.type == "cpu" else a).T

    @classmethod
    def stats(cls, reset: bool = False):
        """{"uploads", "fetches", "bytes_up", "bytes_down"} of every DeviceMatrix since the last reset."""
        out = dict(cls._stats)
        if reset:
            for k in cls._stats:
                cls._stats[k] = 0
        return out


def is_resident(infercnv_obj) -> bool:
    """Does the object carry its matrix as a DeviceMatrix?"""
    return isinstance(infercnv_obj.expr_data, DeviceMatrix)


@dataclass
class InfercnvObject:
    expr_data: np.ndarray                                   # genes x cells, float64 -- or a DeviceMatrix (to_device())
    gene_order: GeneOrder
    reference_grouped_cell_indices: Dict[str, np.ndarray] = field(default_factory=dict)
    observation_grouped_cell_indices: Dict[str, np.ndarray] = field(default_factory=dict)
    count_data: Optional[np.ndarray] = None
    tumor_subclusters: Optional[dict] = None                # {"subclusters": {group: {name: idx}}}
    options: dict = field(default_factory=dict)
    hspike: Optional["InfercnvObject"] = None               # R slot `.hspike`
    gene_names: Optional[np.ndarray] = None                 # rownames(expr.data)
    cell_names: Optional[np.ndarray] = None                 # colnames(expr.data)

    def genes(self):
        return self.gene_names if self.gene_names is not None else np.array(
            [f"gene_{i + 1}" for i in range(self.expr_data.shape[0])])

    def cells(self):
        return self.cell_names if self.cell_names is not None else np.array(
            [f"cell_{i + 1}" for i in range(self.expr_data.shape[1])])

    # ---- helpers mirroring R/inferCNV.R ------------------------------------
    def has_reference_cells(self) -> bool:
        """has_reference_cells (R/inferCNV.R:510-514)."""
        return len(self.reference_grouped_cell_indices) > 0

    def get_reference_grouped_cell_indices(self) -> np.ndarray:
        """unlist(reference_grouped_cell_indices) (R/inferCNV.R:517-520)."""
        if not self.reference_grouped_cell_indices:
            return np.zeros(0, dtype=np.int32)
        return np.concatenate([np.asarray(v, dtype=np.int32) for v in self.reference_grouped_cell_indices.values()])

    def ref_groups_or_proxy(self) -> List[np.ndarray]:
        """Reference groups, or one 'proxyNormal' group of all observation cells
        when no references exist (R/inferCNV_ops.R:1683-1688)."""
        if self.has_reference_cells():
            return [np.asarray(v, dtype=np.int32) for v in self.reference_grouped_cell_indices.values()]
        return [np.concatenate([np.asarray(v, dtype=np.int32)
                                for v in self.observation_grouped_cell_indices.values()])]

    def chr_layout(self):
        """(perm, chr_start): `perm` gathers genes into per-chromosome contiguous
        blocks in order of first appearance (unique(gene_order$chr)); identity when
        the object is already ordered (.order_reduce, R/inferCNV.R:352-428)."""
        chrs = np.asarray(self.gene_order.chr)
        _, first, inv = np.unique(chrs, return_index=True, return_inverse=True)
        rank_of_code = np.argsort(np.argsort(first))          # code -> order of first appearance
        key = rank_of_code[inv]
        perm = np.argsort(key, kind="stable")
        sizes = np.bincount(key, minlength=first.size)
        chr_start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        identity = bool(np.all(perm == np.arange(perm.size)))
        return (None if identity else perm), chr_start

    def copy(self) -> "InfercnvObject":
        return copy.copy(self)

    # ---- device residency (DESIGN K32) --------------------------------------
    def is_resident(self) -> bool:
        return isinstance(self.expr_data, DeviceMatrix)

    def to_device(self, device=None) -> "InfercnvObject":
        """A copy of the object whose expr_data -- and the hspike's with it -- is a DeviceMatrix on `device` (default: the
        current CUDA device).  count_data and all metadata stay where they are.  A resident object is returned as it is."""
        new = self.copy()
        if not isinstance(self.expr_data, DeviceMatrix):
            new.expr_data = DeviceMatrix.from_host(self.expr_data, "expr", device)
        if self.hspike is not None:
            new.hspike = self.hspike.to_device(device)
        return new

    def to_host(self) -> "InfercnvObject":
        """The inverse of to_device(): expr_data (and the hspike's) as the F-ordered float64 host array."""
        new = self.copy()
        if isinstance(self.expr_data, DeviceMatrix):
            new.expr_data = self.expr_data.to_host()
        if isinstance(self.count_data, DeviceMatrix):           # (the counts of a spike-in that was simulated on the device)
            new.count_data = self.count_data.to_host()
        if self.hspike is not None:
            new.hspike = self.hspike.to_host()
        return new

    def validate(self):
        """validate_infercnv_obj (R/inferCNV.R:471-505), the checks relevant here."""
        G, C = self.expr_data.shape
        if np.asarray(self.gene_order.chr).shape[0] != G:
            raise ValueError("gene_order rows must match expr_data rows")
        for name, idx in list(self.reference_grouped_cell_indices.items()) + \
                list(self.observation_grouped_cell_indices.items()):
            idx = np.asarray(idx)
            if idx.size and (idx.min() < 0 or idx.max() >= C):
                raise ValueError(f"cell indices of group {name!r} out of range")
        return True
