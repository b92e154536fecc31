#!/usr/bin/env python3
"""Golden submissions by CALLING the reference's own pose_estimator.test_and_submit (pose_estimator.py:217-318), whose rows its
own submission.SubmissionWriter exports.

Runs only in the build container (needs the reference tree); tests/golden/submit.npz is committed and is the only thing that
travels.  Made the way make_eval_golden.py makes eval.npz: pose_estimator is imported with stub modules, a stub model's `detect`
returns the raw outputs already stored in tests/golden/eval.npz, and each case's images are split into a "virtual" and a "real"
stub dataset whose file names are not in sorted order.  test_and_submit runs in a temporary directory; the text of the
submission_debug.csv it exports is stored per case, with the file names and the image of eval.npz each one belongs to, and the
scalars the reference handed its writer (recorded by wrapping SubmissionWriter._append for the call; float32 values are stored
exactly as float64, with the name of their type), in the order they were appended.

Cases: quaternion, euler, angle_axis, soft_n8, soft_n16.  loc_class and keypoints cannot run through the reference's function
(it hands csv a 1x3 np.matrix inside a list, and it has no keypoint branch); tests/test_predict_gpu.py covers them by bit
equality with urso_pose_eval instead.  No image is left out.

The raw outputs are fp32 values.  detect returns the location and the quaternion / logits as float32 arrays, as Keras does, so
the reference writes them as float32 text.  The Euler angles and the angle-axis vector are handed over as float64 arrays of those
values, as make_eval_golden.py does: that is what the reference's NumPy (1.x) computes when it multiplies a float32 scalar by a
Python float.

    python tests/golden/make_submit_golden.py
"""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, OUT)
from make_eval_golden import BETA, import_reference  # noqa: E402

CASES = ("quaternion", "euler", "angle_axis", "soft_n8", "soft_n16")


class Cfg(object):
    def __init__(self, regress_ori, param, bins):
        self.REGRESS_LOC, self.REGRESS_ORI, self.REGRESS_KEYPOINTS = True, regress_ori, False
        self.ORIENTATION_PARAM, self.BETA, self.ORI_BINS_PER_DIM = param, BETA, bins


class Model(object):
    def __init__(self, config, outs):
        self.config, self.outs = config, outs

    def detect(self, images, verbose=0):
        return [self.outs[int(images[0])]]


class Data(object):
    """image ids 0 .. len - 1; load_image returns the index of the image in the case."""

    def __init__(self, rows, names, hq):
        self.image_ids = list(range(len(rows)))
        self.rows, self.ori_histogram_map = rows, hq
        self.image_info = [{"path": "/data/speed/images/%s" % n} for n in names]

    def load_image(self, i):
        return np.array(self.rows[i])


def main():
    sys.path.insert(0, ROOT)
    from ursonet_amd.pose import OrientationCodec
    pe, _, _ = import_reference()
    g = np.load(os.path.join(OUT, "eval.npz"))
    rng = np.random.default_rng(20261016)
    store = {"cases": np.array(CASES)}
    for c in CASES:
        regress_ori = bool(g[c + "/config"][1])
        param = str(g[c + "/ori_param"])
        loc, ori = g[c + "/loc"], g[c + "/ori"]
        n = len(loc)
        wide = regress_ori and param in ("euler_angles", "angle_axis")
        outs = [{"loc": loc[i].astype(np.float32), "ori": ori[i].astype(np.float64 if wide else np.float32)} for i in range(n)]
        bins = int(g[c + "/ori_bins"]) if not regress_ori else 8
        hq = None if regress_ori else OrientationCodec(bins, BETA).H_quat
        order = rng.permutation(n)                                       # which image goes where, and under which (unsorted) name
        nv = (n + 1) // 2
        rows_v, rows_r = [int(i) for i in order[:nv]], [int(i) for i in order[nv:]]
        def names(fmt, count):                                           # distinct, and not in sorted order
            while True:
                out = [fmt % k for k in rng.permutation(1000)[:count]]
                if out != sorted(out):
                    return out
        names_v, names_r = names("img%06d.jpg", len(rows_v)), names("img%06dreal.jpg", len(rows_r))
        model = Model(Cfg(regress_ori, param, bins), outs)
        import submission as ref_submission
        seen = {False: [], True: []}
        inner = ref_submission.SubmissionWriter._append

        def record(self, filename, q, r, real):
            seen[real].append((filename, list(q), list(r)))
            return inner(self, filename, q, r, real)
        cwd = os.getcwd()
        with tempfile.TemporaryDirectory() as td:
            os.chdir(td)
            try:
                ref_submission.SubmissionWriter._append = record
                with contextlib.redirect_stdout(io.StringIO()):
                    pe.test_and_submit(model, Data(rows_v, names_v, hq), Data(rows_r, names_r, hq))
                with open("submission_debug.csv", newline="") as f:
                    text = f.read()
            finally:
                ref_submission.SubmissionWriter._append = inner
                os.chdir(cwd)
        for real, tag, names in ((False, "virtual", names_v), (True, "real", names_r)):
            assert [t[0] for t in seen[real]] == names
            for k, key in ((1, "q"), (2, "r")):
                kinds = {type(v) for t in seen[real] for v in t[k]}
                f32 = kinds == {np.float32}
                assert f32 or kinds <= {float, np.float64}, kinds
                store["%s/%s_%s" % (c, key, tag)] = np.array([[float(v) for v in t[k]] for t in seen[real]], dtype=np.float64)
                store["%s/%s_dtype" % (c, key)] = "float32" if f32 else "float64"
        store[c + "/csv"] = np.array(text)
        store[c + "/names_virtual"], store[c + "/names_real"] = np.array(names_v), np.array(names_r)
        store[c + "/rows_virtual"], store[c + "/rows_real"] = np.array(rows_v), np.array(rows_r)
        print("%-12s %d + %d images, %d bytes of CSV" % (c, len(rows_v), len(rows_r), len(text)))
    path = os.path.join(OUT, "submit.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes; eval.npz has", os.path.getsize(os.path.join(OUT, "eval.npz")))


if __name__ == "__main__":
    main()
