"""Drop-in for the reference's `pose_estimator.evaluate(model, dataset)` (pose_estimator.py:321-460), batched on the GPU.

The reference runs one image at a time: detect at batch 1, a device-to-host read, NumPy / Python decoding of the configured head
(the soft-classification weighted average alone takes 40-318 ms per image) and the three error formulas.  Here the dataset goes
through the model at its engine batch (IMAGES_PER_GPU; 1 reproduces the reference's batching): EvalFeeder (ordered, no augmentation,
side-stream double buffer) feeds the pass of ursonet_amd/infer.py, whose urso_pose_eval writes each image's estimate and errors into
one fp64 device table.  The table is read once, at the end.

Divergences from the reference, all deliberate:
  * no per-image lines are printed (the reference prints the image id, detect's log and both errors for every image);
  * the arccos argument is clipped to 1 (pose.pose_errors' convention); the reference returns NaN there;
  * `Mean encoded location error` prints nan in regression mode without NumPy's empty-slice warning;
  * the encoded targets are the dataset's stored ones: load_image_gt may draw an augmentation for them (ROT_AUG / ROT_IMAGE_AUG /
    SIM2REAL_AUG), evaluation never does;
  * under a launcher (world > 1) every process evaluates the whole dataset; there is no sharding.
"""
import os

import numpy as np

from .calibrate import check_calibration
from .conformal import bound_fields, check_conformal, no_bound_fields
from .domain import check_domain, domain_fields, no_domain_fields
from .ensemble import EnsemblePass, Members, eval_fields, no_member_fields
from .infer import PosePass, eval_columns, fuse_columns, head_modes, loader_workers  # noqa: F401  (head_modes: its long-standing home is here)

SUMMARY = ("Mean est. location error: ", "Mean est. orientation error: ", "ESA score: ", "Mean encoded location error: ")
CSV_FILES = ("ori_err.csv", "loc_err.csv", "dists_err.csv")


class EvalResult(object):
    """Per-image NumPy arrays in dataset.image_ids order: image_ids, loc_est [N,3], q_est [N,4] ([x, y, z, w]), loc_err, ori_err
    (degrees), esa, dist (loc_gt[2]); loc_encoded_err (location classification) and ori_encoded_err (soft classification), else None;
    with multimodal, ori_err_soft (the soft-argmax estimate's error) and mode (index of the selected mode), else None.  The four
    summary means are computed on the host in fp64 from these arrays.  With views (fused=True: `table` is a FUSE table) the
    estimate and its four errors are the fused pose's, loc_spread, ori_spread (degrees), view_lambda and n_views say how well the views
    agree (else None), and the encoded errors, which do not depend on the estimate, are None.  With members (ensemble: an
    ensemble.EnsembleTables; `table` is not used) the estimate and its errors are the ensemble's, and n_members, member_loc_spread,
    member_ori_spread, member_lambda and the entropies (ori_entropy, ori_member_entropy, ori_mi, loc_entropy, loc_member_entropy,
    loc_mi) are set as on a PredictResult; else they are None.  With conformal (a conformal.Conformal; conformal_tables: the pass's score
    and bound rows): ori_bound / loc_bound and the region fields as on a PredictResult, and ori_covered / loc_covered: whether the error is
    within the bound -- for a classification head taken through the keys (the image's score is at most the level), which is exact; else None.
    With domain (a domain.Domain; domain_table: the pass's score rows): domain_score, domain_dist2, domain_zmax, domain_zarg and domain_p
    as on a PredictResult; else None."""

    def __init__(self, image_ids, table, loc_enc, ori_enc, multimodal, fused=False, *, ensemble=None, conformal=None, conformal_tables=None,
                 domain=None, domain_table=None):
        from . import hip
        self.image_ids = np.asarray(image_ids)
        self.loc_spread = self.ori_spread = self.view_lambda = self.n_views = None
        no_member_fields(self)
        no_bound_fields(self, truth=True)
        no_domain_fields(self)
        if domain is not None:
            domain_fields(self, domain, domain_table)
        if ensemble is not None:
            eval_fields(self, ensemble, loc_enc, ori_enc, multimodal)
            self.dist = ensemble.fuse[:, hip.FUSE_DIST].copy()
            return
        if fused:
            fuse_columns(self, table, True)
            self.loc_encoded_err = self.ori_encoded_err = self.ori_err_soft = self.mode = None
            return
        t = eval_columns(self, table, loc_enc)
        self.esa, self.dist = t[:, hip.EVAL_ESA].copy(), t[:, hip.EVAL_DIST].copy()
        self.ori_encoded_err = t[:, hip.EVAL_ORI_ENC_ERR].copy() if ori_enc else None
        self.ori_err_soft = t[:, hip.EVAL_ORI_ERR_SOFT].copy() if multimodal else None
        self.mode = t[:, hip.EVAL_MODE].astype(np.int32) if multimodal else None
        if conformal is not None:
            bound_fields(self, conformal, conformal_tables, len(self.image_ids), truth=True)

    def means(self):
        """The reference's four printed values (:451-454), in order."""
        enc = self.loc_encoded_err if self.loc_encoded_err is not None else np.zeros(0)
        return [np.mean(self.loc_err), np.mean(self.ori_err), np.mean(self.esa), np.mean(enc) if len(enc) else np.float64(np.nan)]


def summary_lines(means):
    """The text of the reference's four summary prints (:451-454): print(label, value) puts a space between the two."""
    return ["%s %s" % (label, v) for label, v in zip(SUMMARY, means)]


def csv_text(values):
    """pd.DataFrame(np.asarray(values)).to_csv() (:457-459) as text; written by hand with the same format where pandas does not import."""
    a = np.asarray(values)
    try:
        import pandas as pd
    except ImportError:
        return ",0\n" + "".join("%d,%s\n" % (i, "" if np.isnan(v) else str(v)) for i, v in enumerate(a.reshape(-1)))
    return pd.DataFrame(a).to_csv()


def write_csvs(out_dir, ori_err, loc_err, dist):
    """ori_err.csv, loc_err.csv and dists_err.csv in out_dir (:457-459); returns their paths."""
    paths = []
    for name, v in zip(CSV_FILES, (ori_err, loc_err, dist)):
        p = os.path.join(out_dir, name)
        with open(p, "w", newline="") as f:
            f.write(csv_text(v))
        paths.append(p)
    return paths


def ensemble_line(res):
    """The line evaluate(members=...) prints behind the four of the reference: the mean mutual information of each classification head
    (nats) and the mean spread of the members' decoded poses."""
    mi = ["%s MI %s" % (k, np.mean(v)) for k, v in (("orientation", res.ori_mi), ("location", res.loc_mi)) if v is not None]
    return "Ensemble of %d members: mean %smember spread %s (location) %s deg (orientation)" % (
        res.n_members, "".join(m + ", " for m in mi), np.mean(res.member_loc_spread), np.mean(res.member_ori_spread))


def evaluate(model, dataset, multimodal=False, out_dir=".", verbose=1, workers=None, cache=None, views=None, members=None, max_gb=16,
             calibration=None, conformal=None, domain=None):
    """pose_estimator.evaluate(model, dataset): prints the reference's four summary lines (verbose > 0), writes ori_err.csv,
    loc_err.csv and dists_err.csv into out_dir and returns an EvalResult.  multimodal=True (soft classification only) fits up to
    three orientation modes per image (urso_quat_gmm_fit: var = (BETA / ORI_BINS_PER_DIM)^2 / 12, 5 iterations, nr_max_modes 4) and
    takes mode 0 if it is the only one or closer to the truth than mode 1, else mode 1 (the commented block of :410-426).
    cache: a frame_cache.FrameCache of the caller's (Config.DEVICE_RESIZE only) that keeps this dataset's raw frames on the device, so
    that the next call with it -- the next checkpoint, say -- loads no image again; the table is the same with and without it.
    views: [V,3] (pitch, yaw, roll) in degrees, as in predict(): the estimate and its errors are those of the pose fused from V rotated
    views of every image, and the result says how well the views agree; the encoded errors are not computed (run without views for
    them: the fourth line prints nan).  ValueError as in predict().
    members, max_gb: as in predict() -- the estimate and its errors are those of the Bayesian model average of the listed weight sets
    (the same estimate bits as predict(members=...)), the summary lines and CSV files are made from it, and one more line prints the
    mean mutual information and the mean spread of the members.  multimodal fits the modes on the averaged PMF.
    calibration: as in predict() -- the classification heads are decoded from their temperature-scaled logits (the same estimate bits as
    predict(calibration=...)), and one more line prints the temperatures.  Not with members.
    conformal: as in predict() -- the same bound bits as predict(conformal=...); urso_conf_score runs beside urso_conf_bound, the result
    says per image whether the error is within the bound, and one more line prints the target, the empirical coverage and the mean and
    median bound per head.  Not with members, views or multimodal (which picks the mode by the truth: not the estimate the levels are for).
    domain: as in predict() -- the same score bits as predict(domain=...), and one more line prints the median and the 95th percentile of
    the score, with a holdout the share of images with p < 0.05, and Spearman's rho of the score with ori_err and with loc_err.  Not with
    members or views, nor under a data-parallel launcher."""
    check_calibration(calibration, members, "evaluate")
    check_conformal(conformal, members, views, calibration, "evaluate")
    check_domain(domain, members, views, "evaluate")
    if conformal is not None and multimodal:
        raise ValueError("evaluate: conformal=... cannot be combined with multimodal=True: the mode is picked by the truth, and the levels "
                         "were fitted on the soft-argmax estimate")
    if members is not None:
        ms = Members(members, views, "evaluate")
        out, loc_dtype = EnsemblePass(model, dataset, ms, multimodal, True, "evaluate", workers, cache, max_gb).run()
        cfg = model.config
        res = EvalResult(list(dataset.image_ids), None, not cfg.REGRESS_LOC, not (cfg.REGRESS_ORI or cfg.REGRESS_KEYPOINTS), multimodal, ensemble=out)
        if verbose:
            for line in summary_lines(res.means()) + [ensemble_line(res)]:
                print(line)
        write_csvs(out_dir, res.ori_err, res.loc_err, res.dist.astype(loc_dtype) if loc_dtype is not None else res.dist)
        return res
    vs = None
    if views is not None:
        from .views import ViewSet
        vs = ViewSet(views, multimodal, "evaluate").with_camera(dataset, model.config)
    ps = PosePass(model, dataset, multimodal, views=vs, calibration=calibration, conformal=conformal, domain=domain)
    from . import hip
    from .feeder import EvalFeeder
    ids = list(dataset.image_ids)
    N = len(ids)
    table = ps.table(max(N, 1), hip.EVAL_COLS if vs is None else hip.FUSE_COLS)
    gmm = ps.gmm_buffers(ps.B) if multimodal else None
    feed = EvalFeeder(model, dataset, ps.cfg, enc_loc=ps.loc_class and vs is None, enc_ori=ps.soft and vs is None,
                      workers=loader_workers(ps.cfg, workers), cache=cache)
    try:
        for bt in feed:
            if vs is not None:
                ps.fuse_batch(table, bt)
                continue
            ps.run(bt.images)
            ps.domain_scores(table, bt.n, bt.row0)
            heads = ps.heads(bt.n, gmm)
            ps.eval_into(table, bt, heads, gmm)
            ps.bounds(table, bt.n, bt.row0, heads, bt)
    finally:
        feed.close()
    host = table[:N].cpu().numpy()                                              # the one device-to-host read
    res = EvalResult(ids, host, ps.loc_class, ps.soft, multimodal, fused=vs is not None, conformal=conformal,
                     conformal_tables=ps.conformal_tables(N) if conformal is not None else None, domain=domain,
                     domain_table=ps.domain_table(N) if domain is not None else None)
    if verbose:
        for line in (summary_lines(res.means()) + ([calibration.line()] if calibration is not None else []) +
                     ([conformal.line(res)] if conformal is not None else []) + ([domain.line(res)] if domain is not None else [])):
            print(line)
    dist = res.dist.astype(feed.loc_dtype) if feed.loc_dtype is not None else res.dist
    write_csvs(out_dir, res.ori_err, res.loc_err, dist)
    return res
