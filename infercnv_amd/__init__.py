"""infercnv_amd -- MI355X-native hot path of inferCNV (smoothing chain, i6/i3
HMM Viterbi, 2-D median denoise) behind the reference's step-function API.

Host mirror of the R functions: `ops`, `hmm`, `noise_reduction`
(InfercnvObject in, InfercnvObject out).  Device-resident API: `device`.
Cell-sharded multi-GPU: `sharded`.  `run` (pipeline.py) is the driver a
user calls: infercnv::run's 22 steps over those mirrors, from an infercnv
object to CNV calls.  All compute is in libicnv_hip.so
(hand-written HIP for gfx950); there is no CPU fallback.
"""
from ._lib import IcnvError, LIB_PATH, load  # noqa: F401
from .infercnv_object import DeviceMatrix, GeneOrder, InfercnvObject  # noqa: F401
from .create_object import CreateInfercnvObject  # noqa: F401
from .pipeline import run  # noqa: F401
from .sampling import plot_per_group, sample_object, sample_plan  # noqa: F401
from .tumor_subclusters import plot_subclusters  # noqa: F401
from .rds import load_infercnv_obj, save_infercnv_obj  # noqa: F401

__all__ = ["IcnvError", "LIB_PATH", "load", "GeneOrder", "InfercnvObject", "DeviceMatrix", "CreateInfercnvObject", "run",
           "sample_object", "sample_plan", "plot_per_group", "plot_subclusters", "save_infercnv_obj", "load_infercnv_obj"]
