"""The one inference pass under evaluate(), predict(), detect_dataset() and track(): everything between "a batch of frames is on the
device" and "this batch's rows are in the table".  A command builds one PosePass per call and, per batch, on the current stream:
  * run(images) uploads the batch by dtype and replays the inference graph as it is;
  * heads() splits the engine's outputs and, for the soft-classification head, runs urso_quat_wavg_decode on its logits (with the scatter
    matrix only for the DEC table, whose ORI_LAMBDA needs it: passing one selects another kernel variant) and, asked to, urso_quat_gmm_fit;
    with a calibration (ursonet_amd/calibrate.py) the classification heads' logits first go through urso_temp_scale into buffers of the pass's;
  * eval_into() (labelled: estimates and errors, urso_pose_eval, EVAL columns) or decode_into() (no truth: estimates and confidences,
    urso_pose_decode, DEC columns) decodes every head and writes one fp64 row per image into a device table of the caller's.
The two kernels share their device routines, so LOC_EST / Q_EST are the same bits whichever command produced them.  With views
(ursonet_amd/views.py: predict / evaluate, views=...) fuse_batch() takes the place of the three: it runs the batch once per view, warped
on the device, decodes every view into a table of the pass's and ends with one urso_pose_fuse_views into the caller's table.  With a
domain (ursonet_amd/domain.py) domain_scores() pools the batch's bottleneck features and scores them behind run().  Nothing here
synchronises or reads back, and torch, hip and the engine are touched only after check_heads() has passed (no GPU is needed to be
refused).  The commands own their feeders, tables, GMM buffers, result types, prints, files and pictures.
"""
import os

import numpy as np

# the multimodal fit of pose_estimator.py:333-334, :410-426: 5 EM iterations, nr_max_modes 4 (which fits 1 .. 3 modes: 3 slots per image)
GMM_MODES, GMM_ITERATIONS, GMM_MAX_MODES = 3, 5, 4


def head_modes(config):
    """(loc_mode, ori_mode) of urso_pose_eval for a config."""
    from . import hip
    loc_mode = hip.EVAL_LOC_REGRESS if config.REGRESS_LOC else hip.EVAL_LOC_CLASS
    if config.REGRESS_KEYPOINTS:
        return loc_mode, hip.EVAL_ORI_KEYPOINTS
    if not config.REGRESS_ORI:
        return loc_mode, hip.EVAL_ORI_SOFT
    return loc_mode, {"quaternion": hip.EVAL_ORI_QUAT, "euler_angles": hip.EVAL_ORI_EULER,
                      "angle_axis": hip.EVAL_ORI_ANGLE_AXIS}[config.ORIENTATION_PARAM]


def check_heads(model, dataset, multimodal, who="evaluate"):
    """Refuses what the pass cannot run; returns whether the orientation head is the soft-classification one."""
    assert model.mode == "inference", "Create model in inference mode."
    cfg = model.config
    soft = not (cfg.REGRESS_ORI or cfg.REGRESS_KEYPOINTS)
    if multimodal and not soft:
        raise ValueError("%s(multimodal=True) needs the soft-classification orientation head (REGRESS_ORI = False)" % who)
    if not cfg.REGRESS_LOC and getattr(dataset, "histogram_3D_map", None) is None:
        raise ValueError("location classification (REGRESS_LOC = False) needs dataset.histogram_3D_map, the bin map the location "
                         "head was trained on")
    if soft and getattr(dataset, "ori_histogram_map", None) is None:
        raise ValueError("orientation classification (REGRESS_ORI = False) needs dataset.ori_histogram_map")
    if cfg.REGRESS_KEYPOINTS and not cfg.REGRESS_LOC:
        raise ValueError("keypoint evaluation needs a regressed location (REGRESS_LOC = True)")
    return soft


def loader_workers(cfg, workers=None):
    """The number of loader threads: the caller's, else Config.LOADER_WORKERS, else min(8, cpu_count)."""
    return int(getattr(cfg, "LOADER_WORKERS", min(8, os.cpu_count() or 1))) if workers is None else workers


def refuse_launcher(model, who, reason):
    """ValueError under a data-parallel launcher (WORLD_SIZE > 1, or a model built under one; model may be None): the commands that walk
    a whole dataset in one process.  `reason` is what each rank would do."""
    if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 or getattr(model, "_dp", None) is not None or int(getattr(model, "_world", 1)) > 1:
        raise ValueError("%s is not supported under a data-parallel launcher: each rank would %s; run it in a plain process" % (who, reason))


class Subset(object):
    """`dataset` with image_ids cut to the chosen ones; everything else is the dataset's."""

    def __init__(self, dataset, ids):
        self._dataset, self.image_ids = dataset, list(ids)

    def __getattr__(self, name):
        return getattr(self._dataset, name)


def eval_columns(res, table, loc_class):
    """Sets the fields every result of an EVAL table has on `res`; returns the table as fp64 [N, EVAL_COLS] for the caller's own."""
    from . import hip
    t = np.asarray(table, dtype=np.float64).reshape(-1, hip.EVAL_COLS)
    res.loc_est = t[:, hip.EVAL_LOC_EST:hip.EVAL_LOC_EST + 3].copy()
    res.q_est = t[:, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4].copy()
    res.loc_err, res.ori_err = t[:, hip.EVAL_LOC_ERR].copy(), t[:, hip.EVAL_ORI_ERR].copy()
    res.loc_encoded_err = t[:, hip.EVAL_LOC_ENC_ERR].copy() if loc_class else None
    return t


def dec_columns(res, table, loc_class, soft):
    """Sets the fields every result of a DEC table has on `res` (None where the head does not define them)."""
    from . import hip
    t = np.asarray(table, dtype=np.float64).reshape(-1, hip.DEC_COLS)
    res.loc_est = t[:, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3].copy()
    res.q_est = t[:, hip.DEC_Q_EST:hip.DEC_Q_EST + 4].copy()
    res.loc_peak = t[:, hip.DEC_LOC_PEAK].copy() if loc_class else None
    res.ori_peak = t[:, hip.DEC_ORI_PEAK].copy() if soft else None
    res.ori_lambda = t[:, hip.DEC_ORI_LAMBDA].copy() if soft else None


def fuse_columns(res, table, truth):
    """Sets the fields every result of a FUSE table has on `res` (the errors only with a truth); returns the table as fp64 [N, FUSE_COLS]."""
    from . import hip
    t = np.asarray(table, dtype=np.float64).reshape(-1, hip.FUSE_COLS)
    res.loc_est = t[:, hip.FUSE_LOC_EST:hip.FUSE_LOC_EST + 3].copy()
    res.q_est = t[:, hip.FUSE_Q_EST:hip.FUSE_Q_EST + 4].copy()
    res.loc_spread, res.ori_spread = t[:, hip.FUSE_LOC_SPREAD].copy(), t[:, hip.FUSE_ORI_SPREAD].copy()
    res.view_lambda, res.n_views = t[:, hip.FUSE_VIEW_LAMBDA].copy(), t[:, hip.FUSE_N_VIEWS].astype(np.int32)
    if truth:
        res.loc_err, res.ori_err = t[:, hip.FUSE_LOC_ERR].copy(), t[:, hip.FUSE_ORI_ERR].copy()
        res.esa, res.dist = t[:, hip.FUSE_ESA].copy(), t[:, hip.FUSE_DIST].copy()
    return t


class PosePass(object):
    """The per-call state of the pass: cfg, eng, B, dev, the head modes and, on the device, the bin maps loc_map (fp64) and hq (fp32),
    q_soft [B,4] and, with scatter=True, urso_quat_wavg_decode's scatter matrices [B,16].  `who`: the command, for check_heads' messages."""

    def __init__(self, model, dataset, multimodal=False, scatter=False, who="evaluate", views=None, calibration=None, conformal=None,
                 domain=None):
        """views: a views.ViewSet with its homographies (with_camera), for fuse_batch().  calibration: a calibrate.Calibration whose
        inverse temperatures heads() applies to the classification heads' logits (urso_temp_scale into buffers of the pass's: the engine's
        outputs stay as they are); None, or a head whose beta is None: nothing is launched for it.  conformal: a conformal.Conformal whose
        levels bounds() applies behind the decode (urso_conf_bound per classification head into tables of the pass's); None: nothing.
        domain: a domain.Domain whose statistics domain_scores() applies behind run() (urso_feat_pool and urso_feat_maha into a table of
        the pass's); None: nothing."""
        self.soft = check_heads(model, dataset, multimodal, who)
        self.domain, self.dom = domain, None
        if domain is not None:
            domain.check_model(model, who=who)
        self.conformal, self.conf = conformal, None
        if conformal is not None:
            from .ensemble import head_bins
            conformal.check_model(*head_bins(model), who=who)
        self.ori_beta = self.loc_beta = self.z_cal = self.loc_cal = None
        if calibration is not None:
            from .ensemble import head_bins
            calibration.check_model(*head_bins(model), who=who)
            self.ori_beta, self.loc_beta = calibration.ori_beta, calibration.loc_beta
        import torch
        from . import hip
        self.torch, self.hip = torch, hip
        cfg, eng = self.cfg, self.eng = model.config, model._engine
        self.loc_mode, self.ori_mode = head_modes(cfg)
        self.loc_class = self.loc_mode == hip.EVAL_LOC_CLASS
        B, dev = self.B, self.dev = eng.B, eng.device
        self.loc_map = self.hq = self.q_soft = self.scatter = self.var = None
        if self.loc_class:
            self.loc_map = torch.as_tensor(np.asarray(dataset.histogram_3D_map, dtype=np.float64)).to(dev).contiguous()
        if self.soft:
            self.hq = torch.as_tensor(np.ascontiguousarray(dataset.ori_histogram_map, dtype=np.float32)).to(dev).contiguous()
            self.q_soft = torch.empty(B, 4, dtype=torch.float32, device=dev)
            if scatter:
                self.scatter = torch.empty(B, 16, dtype=torch.float32, device=dev)
            if multimodal:
                self.var = (cfg.BETA / cfg.ORI_BINS_PER_DIM) ** 2 / 12         # pose_estimator.py:333-334
        self.views = views
        if views is not None:                                                  # on the device: R [V,9], qR [V,4], one warp matrix per view and batch row [V,B,9]
            from .views import is_identity
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).to(dev).contiguous()   # noqa: E731
            self.view_ident = [is_identity(r) for r in views.R]
            self.view_r, self.view_qr = up(views.R.reshape(views.V, 9)), up(views.qR)
            self.view_m = up(np.repeat(views.M[:, None, :], B, axis=1))
            self.view_table = self.table(views.V * B, hip.DEC_COLS)             # view v's rows at [v * B, v * B + n), reused every batch
            self.view_scratch = None                                           # the warped batch, uint8 [B,H,W,3]

    def table(self, rows, cols):
        """A NaN fp64 device table [rows, cols]."""
        return self.torch.full((rows, cols), float("nan"), dtype=self.torch.float64, device=self.dev)

    def gmm_buffers(self, rows, zeroed=False):
        """urso_quat_gmm_fit's outputs for `rows` images: (mean [rows,3,4], var, prior, score [rows,3] fp32, n_modes [rows] int32)."""
        new, f32 = (self.torch.zeros if zeroed else self.torch.empty), dict(dtype=self.torch.float32, device=self.dev)
        return ((new(rows, GMM_MODES, 4, **f32),) + tuple(new(rows, GMM_MODES, **f32) for _ in range(3)) +
                (new(rows, dtype=self.torch.int32, device=self.dev),))

    def run(self, images):
        """Uploads a batch [B,H,W,3] -- uint8 frames as they are, anything else was molded on the host -- and runs the inference graph."""
        if images.dtype == self.torch.uint8:
            self.eng.load_batch_u8(images)
        else:
            self.eng.set_input_u8(False)
            self.eng.load_batch(images)
        self.eng.forward()

    def heads(self, n, gmm=None):
        """After run(): the engine's outputs as (loc, ori, ori2, z): for the soft head z is the logits of the n valid images (it may alias the
        engine's output buffer) and ori their decoded quaternions; gmm: gmm_buffers' tuple, or views of n rows of it, to fit into."""
        loc, rest = self.eng.outputs()
        ori, ori2 = (rest[0], rest[1]) if self.cfg.REGRESS_KEYPOINTS else (rest, None)
        if self.loc_beta is not None:                              # the calibrated location logits, in a buffer of the pass's
            if self.loc_cal is None:
                self.loc_cal = self.torch.zeros(self.B, loc.shape[1], dtype=self.torch.float32, device=self.dev)
            self.hip.temp_scale(self.B, n, self.loc_beta, loc, self.loc_cal)
            loc = self.loc_cal
        z = None
        if self.soft:
            z = ori[:n].contiguous()
            if self.ori_beta is not None:
                if self.z_cal is None:
                    self.z_cal = self.torch.zeros(self.B, z.shape[1], dtype=self.torch.float32, device=self.dev)
                self.hip.temp_scale(n, n, self.ori_beta, z, self.z_cal)
                z = self.z_cal[:n]
            self.hip.quat_wavg_decode(n, z.shape[1], z, self.hq, self.q_soft, self.scatter)
            if gmm is not None:
                self.hip.quat_gmm_fit(n, z.shape[1], z, False, self.hq, self.var, GMM_ITERATIONS, GMM_MAX_MODES, *gmm)
            ori = self.q_soft
        return loc, ori, ori2, z

    def eval_into(self, table, bt, heads, gmm=None):
        """The rows [bt.row0, bt.row0 + bt.n) of an EVAL table from heads() and the EvalFeeder batch bt's truth and encoded targets; with
        gmm (the per-batch buffers heads() fitted into: urso_pose_eval indexes them by batch row) the fitted mode nearer the truth is scored."""
        loc, ori, ori2, _z = heads
        self.hip.pose_eval(self.B, bt.n, bt.row0, self.loc_mode, self.ori_mode, loc, ori, bt.loc_gt, bt.q_gt, table, ori2=ori2,
                           loc_map=self.loc_map, ori_map=self.hq, enc_loc=bt.enc_loc, enc_ori=bt.enc_ori,
                           gmm_mean=gmm[0] if gmm else None, gmm_nmodes=gmm[4] if gmm else None)

    def decode_into(self, table, n, row0, heads):
        """The rows [row0, row0 + n) of a DEC table from heads()."""
        loc, ori, ori2, z = heads
        self.hip.pose_decode(self.B, n, row0, self.loc_mode, self.ori_mode, loc, ori, table, ori2=ori2, loc_map=self.loc_map, ori_logits=z,
                             ori_map_rows=self.hq.shape[0] if self.soft else 0, ori_scatter=self.scatter)

    def bounds(self, table, n, row0, heads, bt=None):
        """With a conformal: behind eval_into / decode_into of the rows [row0, row0 + n) of `table`, urso_conf_bound per classification
        head at the conformal's level, around the estimates just written, into tables of the pass's (as many rows as `table`); with the
        EvalFeeder batch bt's truth, urso_conf_score as well.  conformal_tables() reads them, once, at the end."""
        if self.conformal is None:
            return
        if self.conf is None:
            from .conformal import ConformalPass
            self.conf = ConformalPass(self, table.shape[0], levels=self.conformal, scores=bt is not None)
        self.conf.launch(table, n, row0, heads, bt)

    def conformal_tables(self, N):
        """{head: (score rows or None, bound rows)} of the classification heads on the host ({} where no batch ran)."""
        return {} if self.conf is None else self.conf.tables(N)

    def domain_scores(self, table, n, row0):
        """With a domain: behind run(), the feature rows of the n valid images (urso_feat_pool on Engine.features()) and their scores
        against the domain (urso_feat_maha) into rows [row0, row0 + n) of a table of the pass's (as many rows as `table`).
        domain_table() reads it, once, at the end."""
        if self.domain is None:
            return
        if self.dom is None:
            from .domain import DomainPass
            self.dom = DomainPass(self, table.shape[0], self.domain)
        self.dom.launch(n, row0)

    def domain_table(self, N):
        """The score rows [N, FEAT_COLS] on the host (no rows where no batch ran)."""
        return np.zeros((0, 4)) if self.dom is None else self.dom.table(N)

    def fuse_batch(self, table, bt):
        """The rows [bt.row0, bt.row0 + bt.n) of a FUSE table: the feeder batch bt once per view through the network -- the identity view
        as run() takes it (no warp: the plain path's bits), any other warped by urso_warp_perspective (bilinear, zero border) from bt.images
        into a scratch batch of the pass's -- each decoded into the pass's per-view table, then one urso_pose_fuse_views, with bt's truth
        where the feeder carries labels.  All on the current stream; nothing is read back."""
        torch, hip, B = self.torch, self.hip, self.B
        if bt.images.dtype != torch.uint8:
            raise ValueError("views need uint8 frames (the warp kernel's input); this batch was molded on the host to %s" % bt.images.dtype)
        _B, H, W, Cc = bt.images.shape
        for v in range(self.views.V):
            if self.view_ident[v]:
                self.run(bt.images)
            else:
                if self.view_scratch is None or self.view_scratch.shape != bt.images.shape:
                    self.view_scratch = torch.empty_like(bt.images)
                hip.warp_perspective(B, H, W, Cc, 1, bt.images, self.view_m[v], self.view_scratch)
                self.run(self.view_scratch)
            self.decode_into(self.view_table, bt.n, v * B, self.heads(bt.n))
        hip.pose_fuse_views(B, bt.n, bt.row0, self.view_table, self.view_r, self.view_qr, table, loc_gt=bt.loc_gt, q_gt=bt.q_gt)
