"""Fixture of the connected-regions / speckle-filter tests (tests/golden/speckle.npz).

Dev-time only, like the other make_golden_* scripts; runs on the CPU and needs scipy.  The expected results come from
scipy.sparse.csgraph.connected_components on the edge list of the contract (tests/speckle_cases.py: edges_of), NOT from the
numpy oracle of that file, which tests/test_speckle_cpu.py then checks against this file.  Stored, for every long-path pattern
of speckle_cases.slow_patterns laid out for a 32 x 64 tile at 70 x 200 (serpentines with their turns on tile borders and
corners, the spiral, the scene) and for 4 and 8 neighbours:

  <name>_c<4|8>_labels   (70,200) int32: the smallest row-major index of the pixel's region, -1 where invalid
  <name>_c<4|8>_sizes    (70,200) int32: the region's pixel count, 0 where invalid
  scene_c<4|8>_s<k>_speckle   (70,200) uint8 for max_size k in (1, 8, 64): valid && size <= k
  tile, shape            what the patterns were laid out for
  numpy, scipy           the versions that evaluated all of it

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_speckle.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
SCENE_SIZES = (1, 8, 64)


def main():
    import scipy
    import speckle_cases as S
    th, tw = S.GOLDEN_TILE
    out = {"tile": np.array(S.GOLDEN_TILE, np.int32), "shape": np.array(S.GOLDEN_SHAPE, np.int32)}
    for name, (d, mask, md) in S.slow_patterns(th, tw).items():
        for c in (4, 8):
            labels, sizes = S.regions_scipy(d, md, mask, True, c)
            valid = S.valid_of(d, mask)
            out[f"{name}_c{c}_labels"], out[f"{name}_c{c}_sizes"] = labels[0, 0], sizes[0, 0]
            line = f"{name} c{c}: {len(np.unique(labels[valid]))} regions, the largest of {int(sizes.max())} pixels"
            if name == "scene":
                for k in SCENE_SIZES:
                    speckle = valid & (sizes <= k)
                    out[f"scene_c{c}_s{k}_speckle"] = speckle[0, 0].astype(np.uint8)
                    line += f"; max_size {k}: {100.0 * speckle.mean():.2f} % removed"
            print(line)
    out["numpy"], out["scipy"] = np.array(np.__version__), np.array(scipy.__version__)
    path = os.path.join(GOLD, "speckle.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print(f"speckle.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
