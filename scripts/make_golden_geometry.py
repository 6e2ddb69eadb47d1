"""Fixture of the stereo-geometry tests (tests/golden/geometry.npz, REPORT_geometry.txt).

Dev-time only, like the other make_golden_* scripts; runs on the CPU where the reference checkout is at hand (only its sample
data is read: samples/tartanair/.../depth_left/000000_left_depth.npy).  Stored:

  ta_depth, ta_disp     a 48x64 crop of the reference's sample depth map and the reference's TartanAir expression on it,
                        disparity = -BASELINE * FX / (depth + 1e-8)  (nndepth/data/datasets/tartanair_dataset.py:28,30,239),
                        evaluated as the dataset evaluates it: numpy, an fp32 array and Python scalars
  ta_fx, ta_baseline    FX = 320, BASELINE = 0.25
  ta_back_depth/_valid  the to_depth oracle (tests/geometry_cases.py) on ta_disp, and ta_points, the points oracle on that depth
  lr_<name>_occ/_err    the float64 left-right oracle on the dyadic scenes of geometry_cases.lr_cases (threshold 1 + 2^-7); the
                        script asserts that the float32 evaluation gives the same mask and the same err, and that
                        |err - threshold| >= 2^-10 at every pixel that reaches the comparison
  numpy                 the numpy version that evaluated all of it

    PYTHONDONTWRITEBYTECODE=1 python scripts/make_golden_geometry.py <path of the reference checkout>
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")
SAMPLE = "samples/tartanair/abandonedfactory/abandonedfactory/Easy/P000/depth_left/000000_left_depth.npy"
CROP = (slice(216, 264), slice(288, 352))
TESTS = (
    ("to_depth", "depth bits and valid mask vs the numpy float64 formula rounded once; 2x1x5x7, 1x1x33x130, a batch-strided "
                 "channel slice, both signs, per-sample fx, min_disp, max_depth on a representable boundary, 0 / -0 / subnormal / "
                 "wrong-sign / inf / NaN"),
    ("to_disparity", "bits vs ta_disp (the reference's expression on the crop); the round trip is not asserted exact"),
    ("points", "dense map, compacted rows, gathered features and offsets vs the float64 oracle; 3x1x9x13 with four masks, "
               "2x1x40x70 (11 workgroups of 256 pixels per sample), 1x1x520x510 (1036 workgroup counts for the 1024 threads of the "
               "scan); two runs byte-equal"),
    ("lr_consistency", "mask and finite err vs the float64 oracle on the dyadic scenes; both signs, right_flipped, W = 5, NaN / "
                       "inf / negative / out-of-frame pixels"),
    ("both_views", "the two halves vs slicing one forward of the torch-built 2B batch (RAFT-Stereo at 64x128 direct and graphed, "
                   "CREStereo at 128x192, channel 0); occlusion() vs lr_consistency of those halves"),
)


def main(ref):
    import geometry_cases as G
    out, rep = {}, [f"stereo geometry: closed-form oracles (scripts/make_golden_geometry.py), numpy {np.__version__}"]
    depth = np.load(os.path.join(ref, SAMPLE))
    assert depth.dtype == np.float32 and depth.shape == (480, 640)
    depth = np.ascontiguousarray(np.expand_dims(depth, axis=0)[:, CROP[0], CROP[1]])  # (1,48,64), as the dataset expands it
    BASELINE, FX = G.TARTANAIR_BASELINE, G.TARTANAIR_FX
    disparity = -BASELINE * FX / (depth + 1e-8)  # tartanair_dataset.py:239, verbatim
    assert disparity.dtype == np.float32
    mine = G.to_disparity(depth[None], [FX], BASELINE)[0]
    ndiff = int((mine.view(np.uint32) != disparity.view(np.uint32)).sum())
    rep.append(f"to_disparity: crop rows {CROP[0].start}:{CROP[0].stop}, columns {CROP[1].start}:{CROP[1].stop} of the sample depth "
               f"(depth {depth.min():.4f} .. {depth.max():.4f}); the oracle's fp32 order differs from the reference's expression in "
               f"{ndiff} of {disparity.size} values")
    assert ndiff == 0
    out.update(ta_depth=depth, ta_disp=disparity, ta_fx=np.float64(FX), ta_baseline=np.float64(BASELINE))
    bd, bv = G.to_depth(disparity[None], [FX], BASELINE)
    out.update(ta_back_depth=bd, ta_back_valid=bv)
    K = np.array([[FX, 0, 32.0], [0, FX, 24.0], [0, 0, 1]], np.float32)
    out.update(ta_K=K, ta_points=G.points_map(bd, G.cam_of(K, 1), bv))
    rt = np.abs(bd[0].astype(np.float64) - depth).max()
    rep.append(f"to_depth(to_disparity(z)) on the crop: all {int(bv.sum())} pixels valid, max |z' - z| = {rt:.3e} (two roundings: not "
               "asserted exact)")
    for name, (mL, mR) in G.lr_cases().items():
        occ64, err64 = G.lr(G.stored(mL, "negative"), G.stored(mR, "negative"), G.LR_THRESHOLD, dtype=np.float64)
        occ32, err32 = G.lr(G.stored(mL, "negative"), G.stored(mR, "negative"), G.LR_THRESHOLD, dtype=np.float32)
        fin = np.isfinite(err64)
        margin = float(np.abs(err64[fin] - G.LR_THRESHOLD).min())
        assert margin >= 2.0 ** -10 and np.array_equal(occ32, occ64)
        assert np.array_equal(err32.astype(np.float64), err64, equal_nan=True)
        out[f"lr_{name}_occ"], out[f"lr_{name}_err"] = occ64, err64.astype(np.float32)
        rep.append(f"lr_consistency {name}: {100.0 * occ64.mean():.1f} % occluded, {int(fin.sum())} of {fin.size} pixels reach the "
                   f"comparison, min |err - threshold| = {margin:.6f}, float32 and float64 masks and err identical")
    out["numpy"] = np.array(np.__version__)
    path = os.path.join(GOLD, "geometry.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    rep.append(f"geometry.npz: {len(out)} arrays, {os.path.getsize(path)} bytes")
    rep.append("what the GPU tests (tests/test_gpu_geometry.py) compare; every comparison is an equality, and on the MI355X every one "
               "holds: 0 differing bits, 0 differing mask pixels, equal offsets (the tests print the counts):")
    rep += [f"  {k:15s} {v}" for k, v in TESTS]
    with open(os.path.join(GOLD, "REPORT_geometry.txt"), "w") as f:
        f.write("\n".join(rep) + "\n")
    print("\n".join(rep))


if __name__ == "__main__":
    main(sys.argv[1])
