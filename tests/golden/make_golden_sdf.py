#!/usr/bin/env python3
"""Generates tests/golden/sdf_henge.npz by running the REFERENCE's own validation/utils/createSDF.py on CPU.

The collision map is the synthetic henge (collision.henge_fn: scene.henge_occupancy in the world frame) on createCollisionMap.py's
box, 2 x 2 x 2 samples per cell (collision.occupancy_from_fn) -- the stand-in for the Blender step, which needs the .blend scene.
createSDF.py then runs unmodified with runpy in a temporary directory: it reads collision_map.npy and writes sdf.npy there.

Stored: the map (np.packbits of the C-order bools), its shape and box, the SHA-256 of the reference's sdf.npy file bytes, and
4096 seeded (flat index, value) samples of the field.  tests/test_collision_gpu.py rebuilds the field with the GPU transform
(SignedDistanceField.from_occupancy) and checks both.

    python tests/golden/make_golden_sdf.py --reference <path of the reference checkout>
"""
import argparse
import hashlib
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds validation/utils/createSDF.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "sdf_henge.npz"))
    args = ap.parse_args()
    from nerfsafetyvalidation_amd import collision as CO

    box = CO.collision_map_box()
    occ = CO.occupancy_from_fn(CO.henge_fn, box, 2).numpy()
    script = os.path.join(args.reference, "validation", "utils", "createSDF.py")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        np.save(os.path.join(tmp, "collision_map.npy"), occ)
        os.chdir(tmp)
        try:
            runpy.run_path(script, run_name="__main__")
        finally:
            os.chdir(cwd)
        raw = open(os.path.join(tmp, "sdf.npy"), "rb").read()
        sdf = np.load(os.path.join(tmp, "sdf.npy"))
    assert sdf.shape == box.shape and sdf.dtype == np.float64
    rng = np.random.default_rng(40)
    idx = rng.choice(sdf.size, size=4096, replace=False).astype(np.int64)
    np.savez_compressed(args.out, occupancy_bits=np.packbits(occ.reshape(-1)), shape=np.asarray(box.shape, np.int64),
                        start=np.asarray(box.start, np.float64), granularity=np.float64(box.granularity),
                        sdf_npy_sha256=np.array(hashlib.sha256(raw).hexdigest()), sample_index=idx, sample_value=sdf.reshape(-1)[idx])
    print(f"{args.out}: {int(occ.sum())} of {occ.size} cells occupied, max distance {sdf.max():.4f} m, sdf.npy sha256 "
          f"{hashlib.sha256(raw).hexdigest()}")


if __name__ == "__main__":
    main()
