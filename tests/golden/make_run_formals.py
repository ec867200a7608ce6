#!/usr/bin/env python3
"""Names, order and default-carrying flags of the formals of the reference's run() (R/inferCNV_ops.R:242-348) ->
run_formals.json: what infercnv_amd.run must accept (tests/test_run_host.py).  API surface, not source, extracted like
r_step_function_signatures.json with r_signatures.formals.

usage: make_run_formals.py <path to the reference checkout>"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import r_signatures  # noqa: E402

FILE = "R/inferCNV_ops.R"


def main(ref):
    fm = r_signatures.formals(open(os.path.join(ref, FILE)).read(), "run")
    assert fm, "run <- function(...) not found"
    out = {"run": {"file": FILE, "formals": [a for a, _ in fm], "has_default": [bool(d) for _, d in fm]}}
    with open(os.path.join(HERE, "run_formals.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("run formals:", len(fm))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
