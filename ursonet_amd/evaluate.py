"""Drop-in for the reference's `pose_estimator.evaluate(model, dataset)` (pose_estimator.py:321-460), batched on the GPU.

The reference runs one image at a time: detect at batch 1, a device-to-host read, NumPy / Python decoding of the configured head
(the soft-classification weighted average alone takes 40-318 ms per image) and the three error formulas.  Here the dataset goes
through the model at its engine batch (IMAGES_PER_GPU; 1 reproduces the reference's batching) and, per batch, on one stream:
upload (EvalFeeder: ordered, no augmentation, side-stream double buffer) -> engine.forward() (the inference graph, replayed as it is)
-> [urso_quat_wavg_decode (soft classification) -> urso_quat_gmm_fit (multimodal)] -> urso_pose_eval, which decodes every head
and writes each image's estimate and errors into one fp64 device table.  The table is read once, at the end.

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

SUMMARY = ("Mean est. location error: ", "Mean est. orientation error: ", "ESA score: ", "Mean encoded location error: ")
CSV_FILES = ("ori_err.csv", "loc_err.csv", "dists_err.csv")


class EvalResult(object):
    """Per-image NumPy arrays in dataset.image_ids order: image_ids, loc_est [N,3], q_est [N,4] ([x, y, z, w]), loc_err, ori_err
    (degrees), esa, dist (loc_gt[2]); loc_encoded_err (location classification) and ori_encoded_err (soft classification), else None;
    with multimodal, ori_err_soft (the soft-argmax estimate's error) and mode (index of the selected mode), else None.  The four
    summary means are computed on the host in fp64 from these arrays."""

    def __init__(self, image_ids, table, loc_enc, ori_enc, multimodal):
        from . import hip
        t = np.asarray(table, dtype=np.float64)
        self.image_ids = np.asarray(image_ids)
        self.loc_est = t[:, hip.EVAL_LOC_EST:hip.EVAL_LOC_EST + 3].copy()
        self.q_est = t[:, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4].copy()
        self.loc_err, self.ori_err = t[:, hip.EVAL_LOC_ERR].copy(), t[:, hip.EVAL_ORI_ERR].copy()
        self.esa, self.dist = t[:, hip.EVAL_ESA].copy(), t[:, hip.EVAL_DIST].copy()
        self.loc_encoded_err = t[:, hip.EVAL_LOC_ENC_ERR].copy() if loc_enc else None
        self.ori_encoded_err = t[:, hip.EVAL_ORI_ENC_ERR].copy() if ori_enc else None
        self.ori_err_soft = t[:, hip.EVAL_ORI_ERR_SOFT].copy() if multimodal else None
        self.mode = t[:, hip.EVAL_MODE].astype(np.int32) if multimodal else None

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


def _check(model, dataset, multimodal, who="evaluate"):
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


def evaluate(model, dataset, multimodal=False, out_dir=".", verbose=1, workers=None, cache=None):
    """pose_estimator.evaluate(model, dataset): prints the reference's four summary lines (verbose > 0), writes ori_err.csv,
    loc_err.csv and dists_err.csv into out_dir and returns an EvalResult.  multimodal=True (soft classification only) fits up to
    three orientation modes per image (urso_quat_gmm_fit: var = (BETA / ORI_BINS_PER_DIM)^2 / 12, 5 iterations, nr_max_modes 4) and
    takes mode 0 if it is the only one or closer to the truth than mode 1, else mode 1 (the commented block of :410-426).
    cache: a frame_cache.FrameCache of the caller's (Config.DEVICE_RESIZE only) that keeps this dataset's raw frames on the device, so
    that the next call with it -- the next checkpoint, say -- loads no image again; the table is the same with and without it."""
    soft = _check(model, dataset, multimodal)
    import torch
    from . import hip
    from .feeder import EvalFeeder
    cfg, eng = model.config, model._engine
    loc_mode, ori_mode = head_modes(cfg)
    loc_enc = not cfg.REGRESS_LOC and not cfg.REGRESS_KEYPOINTS
    ids = list(dataset.image_ids)
    N, B, dev = len(ids), eng.B, eng.device
    table = torch.full((max(N, 1), hip.EVAL_COLS), float("nan"), dtype=torch.float64, device=dev)
    loc_map = torch.as_tensor(np.asarray(dataset.histogram_3D_map, dtype=np.float64)).to(dev).contiguous() if loc_enc else None
    hq = q_soft = mean = nm = None
    if soft:
        hq = torch.as_tensor(np.ascontiguousarray(dataset.ori_histogram_map, dtype=np.float32)).to(dev).contiguous()
        q_soft = torch.empty(B, 4, dtype=torch.float32, device=dev)
        if multimodal:
            M = 3
            mean = torch.empty(B, M, 4, dtype=torch.float32, device=dev)
            gv, gp, gs = (torch.empty(B, M, dtype=torch.float32, device=dev) for _ in range(3))
            nm = torch.empty(B, dtype=torch.int32, device=dev)
            var = (cfg.BETA / cfg.ORI_BINS_PER_DIM) ** 2 / 12                      # :333-334
    if workers is None:
        workers = int(getattr(cfg, "LOADER_WORKERS", min(8, os.cpu_count() or 1)))
    feed = EvalFeeder(model, dataset, cfg, enc_loc=loc_enc, enc_ori=soft, workers=workers, cache=cache)
    try:
        for bt in feed:
            if bt.images.dtype == torch.uint8:
                eng.load_batch_u8(bt.images)
            else:
                eng.set_input_u8(False)
                eng.load_batch(bt.images)
            eng.forward()
            loc, rest = eng.outputs()
            ori, ori2 = (rest[0], rest[1]) if cfg.REGRESS_KEYPOINTS else (rest, None)
            n = bt.n
            if soft:
                z = ori[:n].contiguous()
                hip.quat_wavg_decode(n, z.shape[1], z, hq, q_soft)
                if multimodal:
                    hip.quat_gmm_fit(n, z.shape[1], z, False, hq, var, 5, 4, mean, gv, gp, gs, nm)
                ori = q_soft
            hip.pose_eval(B, n, bt.row0, loc_mode, ori_mode, loc, ori, bt.loc_gt, bt.q_gt, table, ori2=ori2, loc_map=loc_map,
                          ori_map=hq if soft else None, enc_loc=bt.enc_loc, enc_ori=bt.enc_ori,
                          gmm_mean=mean if multimodal else None, gmm_nmodes=nm if multimodal else None)
    finally:
        feed.close()
    host = table[:N].cpu().numpy()                                              # the one device-to-host read
    res = EvalResult(ids, host, loc_enc, soft, multimodal)
    if verbose:
        for line in summary_lines(res.means()):
            print(line)
    dist = res.dist.astype(feed.loc_dtype) if feed.loc_dtype is not None else res.dist
    write_csvs(out_dir, res.ori_err, res.loc_err, dist)
    return res
