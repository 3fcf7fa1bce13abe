#!/usr/bin/env python3
"""Writes tests/golden/backward_plans.json: what the host-side size and query entry points of the grid encoder's and the FFMLP's
backward answer over a sweep of shapes (host arithmetic: the library loads and answers without a GPU).

The committed file was produced from a build of the commit BEFORE the backward plans (GridBwdPlan, FfmlpBwdPlan) were introduced,

    NGP_HIP_LIB=<that build>/libngp_hip.so python tests/golden/make_golden_plans.py

with NGP_GRID_MERGE_MIN and NGP_GRID_BIN_FILL_PCT unset; tests/test_abi.py::test_backward_plans_answer_as_before_the_refactor
compares the library under test with it, value by value.  Regenerate it only together with a deliberate change of those answers.
"""
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "backward_plans.json")

GRID = {"B": [0, 16, 4096, 131071, 131072, 1 << 20, 1 << 24, 29491200], "D": [2, 3], "C": [1, 2, 4, 8], "L": [1, 8, 16, 32],
        "dtype": ["f32", "f16"]}
FFMLP = {"B": [0, 16, 64, 128, 4096, 262144, 1 << 24], "input_dim": [16, 32, 48, 64, 80], "hidden_dim": [16, 32, 64, 128, 256],
         "layers": [2, 3, 4, 5]}


def sweep(axes):
    """the shapes of a sweep in the order the recorded values are in: the first axis varies slowest"""
    return itertools.product(*axes.values())


def answers(lib, _lib):
    code = {"f32": _lib.NGP_F32, "f16": _lib.NGP_F16}
    grid = [lib.ngp_grid_encode_backward_workspace(B, D, C, L, code[dt]) for B, D, C, L, dt in sweep(GRID)]
    ffmlp = [[lib.ngp_ffmlp_backward_workspace(*s), lib.ngp_ffmlp_backward_buffer_bytes(*s), lib.ngp_ffmlp_backward_recomputes(*s[1:])]
             for s in sweep(FFMLP)]
    return {"grid_workspace": grid, "ffmlp_workspace_buffer_recomputes": ffmlp}


def main():
    for name in ("NGP_GRID_MERGE_MIN", "NGP_GRID_BIN_FILL_PCT"):
        if name in os.environ:
            sys.exit(f"{name} is set: the golden answers are those of the defaults")
    sys.path.insert(0, ROOT)
    from nerfsafetyvalidation_amd import _lib
    doc = {"grid_axes": GRID, "ffmlp_axes": FFMLP}
    doc.update(answers(_lib.lib(), _lib))
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(doc['grid_workspace'])} grid and {len(doc['ffmlp_workspace_buffer_recomputes'])} FFMLP shapes from {_lib.SO_PATH}")


if __name__ == "__main__":
    main()
