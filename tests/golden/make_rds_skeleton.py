#!/usr/bin/env python3
"""The structure of the R-written infercnv object of the reference, data/infercnv_object_example.rda, as a skeleton without
values -> rds_skeleton_infercnv_object_example.json (run where the reference exists: `python make_rds_skeleton.py
/path/to/reference`).  tests/test_rds_host.py writes the same object with infercnv_amd.rds, decodes that file with the same
reader (oracle/rda.py) and requires the same skeleton.

A skeleton holds, for every item: its kind, its length or shape, the names of its attributes (for an S4 object: its slots)
in order with their own skeletons, the `class` and `package` strings, `dim`, and the names of list elements.  No data
values, no gene or cell names, no factor levels.  The `call` of an hclust is exempt: R stores the language object, this
library writes NULL (infercnv_amd/rds.py)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

import rda  # noqa: E402

NULL_SLOT = "\x01NULL\x01"
OUT = os.path.join(HERE, "rds_skeleton_infercnv_object_example.json")


def _strings(v):
    v = v.value if isinstance(v, rda.RObject) else v
    return [None if s is None else str(s) for s in (v if isinstance(v, list) else np.asarray(v).tolist())]


def skeleton(v, exempt_call=False):
    if v is None:
        return {"kind": "NULL"}
    if isinstance(v, str):
        return {"kind": "NULL slot"} if v == NULL_SLOT else {"kind": "symbol or string"}
    if isinstance(v, np.ndarray):
        return {"kind": str(v.dtype), "shape": list(v.shape)}
    if isinstance(v, list):
        if v and all(e is None or isinstance(e, str) for e in v) and any(isinstance(e, str) for e in v):
            return {"kind": "str", "length": len(v)}
        return {"kind": "list", "length": len(v), "elements": [skeleton(e) for e in v]}
    if isinstance(v, dict):          # a pairlist (a language object decodes as one too)
        return {"kind": "pairlist", "length": len(v)}
    if not isinstance(v, rda.RObject):
        raise TypeError(type(v))
    out = {"kind": v.kind, "attributes": list(v.attrs)}
    classes = _strings(v.attrs["class"]) if "class" in v.attrs else []
    if classes:
        out["class"] = classes
    if "dim" in v.attrs:
        out["dim"] = [int(x) for x in np.asarray(v.attrs["dim"])]
    for name, a in v.attrs.items():
        if name in ("dim",):
            continue
        if name in ("class", "package"):
            sk = {"kind": "str", "strings": _strings(a)}
            if isinstance(a, rda.RObject):
                sk["attributes"] = {k: {"kind": "str", "strings": _strings(b)} for k, b in a.attrs.items()}
        elif name == "names" and v.kind in ("namedlist", "list"):
            sk = {"kind": "str", "strings": _strings(a)}
        elif v.kind == "S4":
            sk = skeleton(a)
        else:
            sk = skeleton(a)
        out.setdefault("attribute_skeletons", {})[name] = sk
    if v.kind == "namedlist":
        out["elements"] = {k: ({"kind": "call (exempt)"} if k == "call" and "hclust" in classes else skeleton(e))
                           for k, e in v.value.items()}
    elif v.kind == "list":
        out["length"] = len(v.value)
        out["elements"] = [skeleton(e) for e in v.value]
    elif v.kind == "matrix":
        out["dtype"] = str(np.asarray(v.value).dtype)
    elif v.kind == "str":
        out["length"] = len(v.value)
    elif v.kind != "S4":
        out["dtype"], out["length"] = str(np.asarray(v.value).dtype), int(np.asarray(v.value).size)
    return out


def decode(path):
    """The top-level item of an .rds file, or the one variable of an .rda container."""
    with open(path, "rb") as fh:
        buf = rda._decompress(fh.read())
    rd = rda._Reader(buf)
    container = buf[:5] in (b"RDX2\n", b"RDX3\n")
    rd.header()
    top = rd.item()
    if container:
        (top,) = top.values()
    return top


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("INFERCNV_REFERENCE", "")
    src = os.path.join(ref, "data", "infercnv_object_example.rda")
    if not os.path.exists(src):
        sys.exit(__doc__)
    with open(OUT, "w") as fh:
        json.dump(skeleton(decode(src)), fh, indent=1, sort_keys=False)
        fh.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
