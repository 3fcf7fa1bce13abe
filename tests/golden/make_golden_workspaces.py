#!/usr/bin/env python3
"""Writes tests/golden/workspace_sizes.json: what every ngp_*_workspace size function whose entry point carves its scratch through
csrc/workspace.hpp answers over a sweep of shapes (host arithmetic: the library loads and answers without a GPU).

The committed file was produced in a checkout of the commit BEFORE the layouts were introduced (each size function a line of
arithmetic of its own), from a build of that commit,

    NGP_HIP_LIB=<that build>/libngp_hip.so python tests/golden/make_golden_workspaces.py

tests/test_abi.py::test_workspace_sizes_answer_as_before_the_layouts compares the library under test with it, value by value.
Regenerate it only together with a deliberate change of those answers.

The sweep holds the edges: 0 and 1; one below, at and above every threshold inside a size function (16384 / 16385 rays for the mean
of the losses and for the train march's trace, 1023 / 1024 rays where the train march starts to use its occupancy copies, 65535 /
65536 rays for the upsample route); sizes that are no multiple of a block granule (a 5 x 6 x 7 lattice); sizes the function refuses
(answer 0); and 2^31 - 1 cells.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_sizes.json")

M31 = (1 << 31) - 1      # a prime: 2^31 - 1 cells is M31 x 1 x 1
RAYS = [0, 1, 63, 64, 65, 16383, 16384, 16385, 16448, 16449, 1 << 20, (1 << 32) - 1]
VOLUMES = [[0, 5, 6], [1, 1, 1], [1, 8, 8], [2, 2, 2], [4, 5, 6], [5, 6, 7], [8, 8, 8], [9, 10, 33], [64, 64, 64], [255, 257, 3], [128, 128, 128],
           [16384, 16384, 1], [2, 2, 536870911], [1290, 1290, 1290], [M31, 1, 1], [2048, 1024, 1024], [65536, 65536, 1]]
CASES = {
    "march_rays_train": [[n] for n in [0, 1, 5, 255, 256, 257, 1023, 1024, 1025, 4096, 16383, 16384, 16385, 65536, 1 << 20, M31, (1 << 32) - 1]],
    "edt_sq": VOLUMES,
    "label_components": VOLUMES,
    "isosurface": VOLUMES,
    "distance_stats": [[n] for n in [0, 1, 63, 64, 65, 130, 1 << 20, M31, 1 << 31, 1 << 40]],
    "render_upsample": [[0, 4, 2], [1, 4, 2], [65535, 4, 2], [65536, 4, 2], [65537, 4, 2], [65551, 3, 1], [65552, 128, 128], [1 << 20, 128, 128],
                        [1 << 20, 512, 512]],
    # (cascade * H^3 >= 2^32 -- H = 1024 with four or more cascades -- is not swept: the old count wrapped there, as the kernels' own 32-bit cell count does)
    "density_grid": [[c, H] for c in range(1, 9) for H in [2, 4, 8, 16, 32, 64, 128, 256, 512]] + [[c, 1024] for c in (1, 2, 3)],
    "uq_stats": [[]],
    "sigma_fit": [[0, 0], [1, 0], [64, 0], [65, 0], [300, 3], [300, 0], [300, 1], [1 << 20, 0], [1 << 20, 4096], [1 << 20, 4097], [(1 << 32) - 1, 0]],
    "image_quality": [[0, 8, 8], [1, 5, 8], [1, 8, 5], [1, 6, 6], [1, 8, 8], [2, 71, 133], [4, 800, 800], [65535, 6, 6], [65536, 6, 6], [1, 32768, 32768],
                      [1, 32769, 8]],
    "sift": [[7, 8], [8, 7], [8, 8], [9, 13], [48, 48], [100, 100], [480, 640], [16384, 8], [16385, 8], [16384, 16384]],
    "photo_loss": [[n] for n in RAYS],
    "distortion": [[n] for n in RAYS],
    "depth_loss": [[n] for n in RAYS],
}

# The one size that changed on purpose.  ngp_density_grid_finish writes cascade * ceil(H^3 / 256) partial sums, one run of workgroups
# per level; the old size function counted ceil(cascade * H^3 / 256).  The two differ only where a level has fewer than 256 cells, H = 2
# and H = 4 with more than one cascade; there the old answer covered the bytes touched only through its 64 spare bytes.  The layout states
# the count the kernels use: new = H^3 * 8 + cascade * ceil(H^3 / 256) * 8 + 64.
DENSITY_GRID_EXCEPTIONS = [{"cascade": c, "H": H, "old": H ** 3 * 8 + -(-c * H ** 3 // 256) * 8 + 64, "new": H ** 3 * 8 + c * 8 + 64,
                            "reason": "one partial sum per level and 256 cells of it, not per 256 cells of all levels"}
                           for c in range(2, 9) for H in (2, 4)]


def answers(lib):
    return {name: [getattr(lib, f"ngp_{name}_workspace")(*args) for args in shapes] for name, shapes in CASES.items()}


def main():
    sys.path.insert(0, ROOT)
    from nerfsafetyvalidation_amd import _lib
    doc = {"cases": CASES, "answers": answers(_lib.lib())}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {sum(len(v) for v in CASES.values())} shapes of {len(CASES)} size functions from {_lib.SO_PATH}")


if __name__ == "__main__":
    main()
