#!/usr/bin/env python3
"""Extract the reference's two stored hclust objects into tests/golden/hclust_example.npz (run where the reference's
data/ directory is readable; GPU machines only see the committed output).

  python tests/golden/make_hclust_golden.py [path/to/infercnv]

data/infercnv_object_example.rda stores @tumor_subclusters$hc$tumor and $normal: ward.D2 hclust objects,
call = hclust(dist(t(tumor_expr_data))), of the step-14 (pre-denoise) matrix of that run restricted to each group's
cells.  Saved per group: merge (n-1, 2) int32, height, order (1-based), labels, method, dist.method.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
import rda  # noqa: E402


def _v(x):
    return x.value if hasattr(x, "value") else x


def main(ref):
    obj = rda.read_rda(os.path.join(ref, "data", "infercnv_object_example.rda"))["infercnv_object_example"]
    hc = _v(_v(obj.attrs["tumor_subclusters"])["hc"])
    out = {}
    for grp in ("tumor", "normal"):
        h = _v(hc[grp])
        out[f"{grp}_merge"] = np.asarray(rda.as_matrix(h["merge"]), dtype=np.int32)
        out[f"{grp}_height"] = np.asarray(_v(h["height"]), dtype=np.float64)
        out[f"{grp}_order"] = np.asarray(_v(h["order"]), dtype=np.int32)
        out[f"{grp}_labels"] = np.array([str(s) for s in _v(h["labels"])])
        out[f"{grp}_method"] = np.array(str(_v(h["method"])[0]))
        out[f"{grp}_dist_method"] = np.array(str(_v(h["dist.method"])[0]))
    np.savez_compressed(os.path.join(HERE, "hclust_example.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
