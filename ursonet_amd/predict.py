"""Poses for images that have no labels, batched on the GPU: the input side of the reference's `submit` command
(pose_estimator.test_and_submit, pose_estimator.py:217-318; the writer is ursonet_amd/submission.py).

evaluate() needs a ground truth for every image (its feeder loads one, urso_pose_eval refuses a null one); the SPEED `test` and
`real_test` splits have none.  predict() walks the dataset the same way -- EvalFeeder with labels=False (only load_image is called)
feeds the pass of ursonet_amd/infer.py -- and ends each batch with urso_pose_decode, which writes each image's estimate and the
confidence of the classification heads into one fp64 device table, read once at the end.  The estimates are the bits evaluate()
produces for the same images.

predict(views=...) shows the network V rotated views of every image (ursonet_amd/views.py) and returns the fused estimate and how well
the views agree -- a confidence the regression heads do not otherwise have (the pass: infer.PosePass.fuse_batch).

Under a launcher (world > 1) every process predicts the whole dataset; there is no sharding.
"""
import numpy as np

from .calibrate import check_calibration
from .conformal import bound_fields, check_conformal, no_bound_fields
from .domain import check_domain, domain_fields, no_domain_fields
from .ensemble import EnsemblePass, Members, no_member_fields, predict_fields
from .infer import PosePass, dec_columns, fuse_columns, loader_workers


class PredictResult(object):
    """Per-image NumPy arrays in dataset.image_ids order: image_ids, loc_est [N,3], q_est [N,4] ([x, y, z, w]) and the confidence
    the heads give without a truth to compare with: loc_peak (location classification: the largest softmax probability of the
    location bins), ori_peak and ori_lambda (soft classification: the largest probability of the orientation bins, and the largest
    eigenvalue of the PMF's scatter matrix sum_i w_i q_i q_i^T -- 1 for a point mass, 1/4 for a uniform spread); None where the
    head does not define them.  With multimodal: modes [N,3,4], mode_priors [N,3] (descending; unused slots 0) and n_modes [N].
    With views (fused=True: `table` is a FUSE table): loc_est / q_est are the fused estimate, loc_spread, ori_spread (degrees: RMS
    deviation of the de-rotated views from it), view_lambda (1 when all views agree, 1/4 for a uniform spread) and n_views are set, and
    loc_peak / ori_peak / ori_lambda, which are per-view quantities, are None.  Without views the four are None.
    With members (ensemble: an ensemble.EnsembleTables; `table` is not used): loc_est / q_est are the ensemble's -- a classification
    head's from the mean of the members' PMFs, a regression head's fused from the members' poses -- loc_peak / ori_peak / ori_lambda are
    those of the averaged PMF, n_members is M, member_loc_spread, member_ori_spread (degrees) and member_lambda say how far the members'
    decoded poses spread (urso_pose_fuse_views' columns), and per classification head, in nats: ori_entropy / loc_entropy (of the averaged
    PMF), ori_member_entropy / loc_member_entropy (the mean of the members') and ori_mi / loc_mi (their difference, the mutual
    information: the epistemic part).  Without members all of these are None.
    With conformal (a conformal.Conformal; conformal_tables: the pass's bound rows): ori_bound (degrees) and loc_bound (metres), the
    error bounds that hold with probability 1 - alpha, and for a classification head ori_region_bins / loc_region_bins (the bins inside the
    bound) and ori_region_mass / loc_region_mass (their PMF mass); None for a regression head, whose bound is a constant.  Without: None.
    With domain (a domain.Domain; domain_table: the pass's score rows): domain_score (the squared Mahalanobis distance of the image's
    pooled bottleneck features to the source domain), domain_dist2 (the squared Euclidean distance to its mean), domain_zmax / domain_zarg
    (the largest whitened component and its index) and domain_p (the conformal p-value against the domain's holdout scores; None without
    a holdout).  Without: None."""

    def __init__(self, image_ids, table, loc_class, soft, gmm=None, fused=False, *, ensemble=None, conformal=None, conformal_tables=None,
                 domain=None, domain_table=None):
        self.loc_spread = self.ori_spread = self.view_lambda = self.n_views = None
        no_member_fields(self)
        no_bound_fields(self)
        no_domain_fields(self)
        if ensemble is not None:
            predict_fields(self, ensemble, loc_class, soft)
        elif fused:
            fuse_columns(self, table, False)
            self.loc_peak = self.ori_peak = self.ori_lambda = None
        else:
            dec_columns(self, table, loc_class, soft)
        self.image_ids = np.asarray(image_ids)
        self.modes, self.mode_priors, self.n_modes = gmm if gmm is not None else (None, None, None)
        if conformal is not None:
            bound_fields(self, conformal, conformal_tables, len(self.image_ids))
        if domain is not None:
            domain_fields(self, domain, domain_table)


def predict(model, dataset, multimodal=False, workers=None, cache=None, views=None, members=None, max_gb=16, calibration=None,
            conformal=None, domain=None):
    """Pose estimates of every image of `dataset` -> PredictResult.  The dataset needs image_ids, load_image, image_info and, for
    the classification heads, histogram_3D_map / ori_histogram_map; no label loader is called.  multimodal=True (soft
    classification only) also fits up to three orientation modes per image (urso_quat_gmm_fit: var = (BETA / ORI_BINS_PER_DIM)^2 /
    12, 5 iterations, nr_max_modes 4) and returns them; without a truth to pick a mode by, q_est stays the soft-argmax estimate.  cache: as in evaluate() -- a
    frame_cache.FrameCache of the caller's that keeps the raw frames on the device between calls (Config.DEVICE_RESIZE only).
    views: [V,3] (pitch, yaw, roll) in degrees, e.g. views.ROLL_VIEWS(3, 30): every image is shown to the network once per view (the
    frame re-rendered through the rotated camera; needs dataset.camera), the estimates are rotated back and fused.  None: one pass, as ever.
    ValueError: views with multimodal, a bad views array, no dataset.camera, IMAGE_RESIZE_MODE 'crop' / 'none'.
    members: 1 .. 64 weight sets of this network (weights files, or {layer: {weight: array}} dicts), e.g. SWAG samples written with
    swag_weights + save_weights: the Bayesian model average (ursonet_amd/ensemble.py).  The dataset is walked once per member; the
    estimate of a classification head is decoded from the mean of the members' PMFs (multimodal: the modes are fitted on it), a regression
    head's is fused from the members' poses, and the result carries the entropies and the members' spread.  The model's own weights are
    back when the call returns or raises.  max_gb: the most device memory the whole-dataset accumulators may take.  ValueError: a bad
    members list, a member that lacks a layer, views with members, accumulators above max_gb (the message names their size).  None: as ever.
    calibration: a calibrate.Calibration (from calibrate(), Calibration.load() or built by hand): the logits of each classification head
    are multiplied by its fitted inverse temperature (urso_temp_scale) before they are decoded, so loc_peak, ori_peak, ori_lambda, the
    modes and the soft-argmax q_est are those of the calibrated PMF; views work, members do not (ValueError: calibrate and predict each
    member on its own), nor does a calibration fitted on other bin counts.  None: the code of before, bit for bit.
    conformal: a conformal.Conformal (from conformal() or Conformal.load()): behind the decode, urso_conf_bound gives every image the
    smallest ball around its estimate that holds more than the fitted level of the head's PMF mass: ori_bound / loc_bound and the region
    fields (a regression head gets its constant).  ValueError: with members or views, under calibration betas other than the ones the
    levels were fitted under (the message names both), bin counts that do not fit the model.  None: nothing is launched.
    domain: a domain.Domain (from fit_domain() or Domain.load()): behind each batch's forward pass urso_feat_pool and urso_feat_maha
    give every image its squared Mahalanobis distance to the source domain's feature statistics: domain_score, domain_dist2,
    domain_zmax, domain_zarg, domain_p.  Works with calibration and conformal.  ValueError: with members or views, under a data-parallel
    launcher, a model of another feature geometry.  None: nothing is launched, the code of before bit for bit."""
    check_calibration(calibration, members, "predict")
    check_conformal(conformal, members, views, calibration, "predict")
    check_domain(domain, members, views, "predict")
    if members is not None:
        ms = Members(members, views, "predict")
        out, _dt = EnsemblePass(model, dataset, ms, multimodal, False, "predict", workers, cache, max_gb).run()
        cfg = model.config
        return PredictResult(list(dataset.image_ids), None, not cfg.REGRESS_LOC, not (cfg.REGRESS_ORI or cfg.REGRESS_KEYPOINTS), out.gmm,
                             ensemble=out)
    vs = None
    if views is not None:
        from .views import ViewSet
        vs = ViewSet(views, multimodal, "predict").with_camera(dataset, model.config)
    ps = PosePass(model, dataset, multimodal, scatter=vs is None, who="predict", views=vs, calibration=calibration, conformal=conformal,
                  domain=domain)
    from . import hip
    from .feeder import EvalFeeder
    ids = list(dataset.image_ids)
    N = len(ids)
    table = ps.table(max(N, 1), hip.DEC_COLS if vs is None else hip.FUSE_COLS)
    gmm = ps.gmm_buffers(max(N, 1), zeroed=True) if multimodal else None          # whole-dataset outputs: each batch fits into its rows
    feed = EvalFeeder(model, dataset, ps.cfg, workers=loader_workers(ps.cfg, workers), labels=False, cache=cache)
    try:
        for bt in feed:
            if vs is not None:
                ps.fuse_batch(table, bt)
                continue
            ps.run(bt.images)
            ps.domain_scores(table, bt.n, bt.row0)
            rows = [t[bt.row0:bt.row0 + bt.n] for t in gmm] if multimodal else None
            heads = ps.heads(bt.n, rows)
            ps.decode_into(table, bt.n, bt.row0, heads)
            ps.bounds(table, bt.n, bt.row0, heads)
    finally:
        feed.close()
    host = table[:N].cpu().numpy()                                               # the one read of the table
    fit = tuple(gmm[i][:N].cpu().numpy() for i in (0, 2, 4)) if multimodal else None      # mean, prior, n_modes
    return PredictResult(ids, host, ps.loc_class, ps.soft, fit, fused=vs is not None, conformal=conformal,
                         conformal_tables=ps.conformal_tables(N) if conformal is not None else None, domain=domain,
                         domain_table=ps.domain_table(N) if domain is not None else None)
