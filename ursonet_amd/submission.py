"""The reference's `submit` command: SubmissionWriter (submission.py) and test_and_submit (pose_estimator.py:217-318) on top of
the batched predict() (ursonet_amd/predict.py).

The submission is one CSV file, one row per image: file name, quaternion [w, x, y, z], location [x, y, z]; the rows of the
synthetic test set come first, then those of the real one, each group sorted by file name; lines end with "\\n".  The csv module
writes every number with str(), so the scalar type decides the text: test_and_submit hands over numpy.float32 scalars where the
reference's value is float32 (the quaternion of the quaternion and soft-classification heads, a regressed location) and
numpy.float64 where the reference computes in float64 (Euler angles, angle-axis, a classified location).

Divergences from the reference, all deliberate:
  * no per-image lines are printed (the reference prints the image id and detect's log for every image);
  * location classification writes three numbers; the reference hands csv a 1x3 np.matrix inside a list and writes one bracketed field;
  * keypoint mode is decoded as evaluate() decodes it; the reference's function has no branch for it and raises;
  * the soft-classification quaternion's sign is normalised (largest-magnitude component positive); the reference's depends on the
    eigen-solver;
  * under a launcher (world > 1) every process predicts both datasets; only rank 0 writes the file.
"""
import csv
import os
from datetime import datetime

import numpy as np


class SubmissionWriter(object):
    """Collects (file name, q, r) rows of the synthetic and the real test set and exports them as submission_<suffix>.csv."""

    def __init__(self):
        self.test_results, self.real_test_results = [], []

    def append_test(self, filename, q, r):
        """One image of the synthetic test set: q = [w, x, y, z], r = location."""
        self.test_results.append((filename, list(q), list(r)))

    def append_real_test(self, filename, q, r):
        """One image of the real test set."""
        self.real_test_results.append((filename, list(q), list(r)))

    def export(self, out_dir='', suffix=None):
        """Writes out_dir/submission_<suffix>.csv (suffix None: the time, %Y%m%d-%H%M) and returns its path."""
        if suffix is None:
            suffix = datetime.now().strftime("%Y%m%d-%H%M")
        path = os.path.join(out_dir, "submission_%s.csv" % suffix)
        by_name = lambda row: row[0]                                             # noqa: E731
        with open(path, "w") as f:
            out = csv.writer(f, lineterminator="\n")
            for name, q, r in sorted(self.test_results, key=by_name) + sorted(self.real_test_results, key=by_name):
                out.writerow([name] + q + r)
        print("Submission saved to %s." % path)
        return path


def scalar_types(config):
    """(quaternion dtype, location dtype) of the values the reference's test_and_submit writes for this head configuration."""
    q64 = config.REGRESS_KEYPOINTS or (config.REGRESS_ORI and config.ORIENTATION_PARAM in ("euler_angles", "angle_axis"))
    return (np.float64 if q64 else np.float32), (np.float32 if config.REGRESS_LOC else np.float64)


def submission_rows(result, dataset, config):
    """[(file name, [w, x, y, z], [x, y, z])] of a PredictResult, in its order, as the scalars the CSV text is made from."""
    qt, lt = scalar_types(config)
    rows = []
    for image_id, q, loc in zip(result.image_ids, result.q_est, result.loc_est):
        name = dataset.image_info[image_id]["path"].split("/")[-1]
        rows.append((name, [qt(q[3]), qt(q[0]), qt(q[1]), qt(q[2])], [lt(v) for v in loc]))
    return rows


def test_and_submit(model, dataset_virtual, dataset_real, out_dir='', suffix='debug', views=None, members=None, calibration=None, conformal=None):
    """pose_estimator.test_and_submit: predicts both label-free datasets, writes submission_<suffix>.csv into out_dir (rank 0
    only) and returns the two PredictResults.  views: as in predict() -- the submitted poses are the ones fused from rotated views.
    members: as in predict() -- the submitted poses are those of the ensemble of the listed weight sets.
    calibration: as in predict() -- the classification heads are decoded from their temperature-scaled logits (not with members).
    conformal: as in predict() -- the two results carry the error bounds (the submission file does not)."""
    from .predict import predict
    res_v = predict(model, dataset_virtual, views=views, members=members, calibration=calibration, conformal=conformal)
    res_r = predict(model, dataset_real, views=views, members=members, calibration=calibration, conformal=conformal)
    from .dp import launcher_world                                               # (behind predict: its refusals need neither torch nor a GPU)
    if launcher_world()[0] == 0:
        sub = SubmissionWriter()
        for row in submission_rows(res_v, dataset_virtual, model.config):
            sub.append_test(*row)
        for row in submission_rows(res_r, dataset_real, model.config):
            sub.append_real_test(*row)
        sub.export(out_dir=out_dir, suffix=suffix)
        print("Submission exported.")
    return res_v, res_r


test_and_submit.__test__ = False                                                 # a command of the driver, not a pytest case
