#!/usr/bin/env python3
"""Golden Unreal Euler angles by CALLING the reference's own se3lib (NumPy only) the way pose_estimator.detect_video does
(pose_estimator.py:669-678).

Needs the reference tree, so it runs only where that exists; tests/golden/video_pose.npz is committed and is the only thing that travels.

    python tests/golden/make_video_golden.py <reference tree>

64 quaternions [x, y, z, w]: 40 random ones and 24 built so that R_wo[2, 0] -- the entry se3lib.SO32euler branches on at +-0.998 --
sits at +-0.9979, +-0.9981 (the thresholds' neighbours at +-1e-4, so that no case lies on a branch boundary), +-0.9995 and +-1, three
of each with different rotations about the two axes that leave that entry alone.  Stored: q, euler = [-pitch, yaw, -roll] exactly as the
reference derives it (`roll, pitch, yaw = se3lib.SO32euler(R_wo)`), r20 = R_wo[2, 0] and branch (+1 / -1: the gimbal-lock branches, 0:
the general one).
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
TARGETS = (0.9979, -0.9979, 0.9981, -0.9981, 0.9995, -0.9995, 1.0, -1.0)


def reference_row(se3lib, q):
    R_cam_unreal = np.matrix([[0, 1, 0], [0, 0, 1], [1, 0, 0]])
    R_co = se3lib.quat2SO3(q)
    R_co = R_cam_unreal.T * R_co
    R_wc = se3lib.euler2SO3_unreal(0, 0, 0)
    R_wo = R_wc * R_co
    roll, pitch, yaw = se3lib.SO32euler(R_wo)
    return [-pitch, yaw, -roll], float(R_wo[2, 0])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.path.insert(0, sys.argv[1])
    import se3lib
    rng = np.random.RandomState(20)
    qs = []
    for _ in range(40):
        q = rng.normal(size=4)
        qs.append(q / np.linalg.norm(q))
    # R_wo[2, 0] = R_co[1, 0].  R_co = Ry(a) . Z(v) . Rx(b) keeps e1^T R e0 = v: Ry fixes e1 from the left, Rx fixes e0 from the right
    for v in TARGETS:
        for _ in range(3):
            a, b = rng.uniform(-np.pi, np.pi, size=2)
            c = np.sqrt(max(0.0, 1 - v * v))
            Z = np.array([[c, -v, 0], [v, c, 0], [0, 0, 1.0]])
            Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
            q = np.asarray(se3lib.SO32quat(np.matrix(Ry @ Z @ Rx)), dtype=np.float64)
            qs.append(q / np.linalg.norm(q))
    qs = np.asarray(qs)
    rows, r20 = zip(*(reference_row(se3lib, q) for q in qs))
    rows, r20 = np.asarray(rows, dtype=np.float64), np.asarray(r20)
    branch = np.where(r20 > 0.998, 1, np.where(r20 < -0.998, -1, 0))
    want = np.repeat(TARGETS, 3)
    assert np.all(np.abs(r20[40:] - want) < 1e-9), r20[40:] - want
    assert np.all(np.abs(np.abs(r20) - 0.998) > 5e-5)
    assert sorted(set(branch[40:])) == [-1, 0, 1] and np.all(np.isfinite(rows))
    np.savez(os.path.join(OUT, "video_pose.npz"), q=qs, euler=rows, r20=r20, branch=branch.astype(np.int64))
    print("wrote video_pose.npz:", qs.shape, "branches", {int(b): int((branch == b).sum()) for b in (-1, 0, 1)})


if __name__ == "__main__":
    main()
