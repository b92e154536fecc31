"""Poses for images that have no labels, batched on the GPU: the input side of the reference's `submit` command
(pose_estimator.test_and_submit, pose_estimator.py:217-318; the writer is ursonet_amd/submission.py).

evaluate() needs a ground truth for every image (its feeder loads one, urso_pose_eval refuses a null one); the SPEED `test` and
`real_test` splits have none.  predict() walks the dataset the same way -- the model's engine batch, one stream, per batch:
upload (EvalFeeder with labels=False: only load_image is called) -> engine.forward() (the inference graph, replayed as it is) ->
[urso_quat_wavg_decode with its scatter matrix (soft classification) -> urso_quat_gmm_fit (multimodal)] -> urso_pose_decode, which
writes each image's estimate and the confidence of the classification heads into one fp64 device table, read once at the end.
The estimates are the bits evaluate() produces for the same images (both kernels share their device routines).

Under a launcher (world > 1) every process predicts the whole dataset; there is no sharding.
"""
import os

import numpy as np

from .evaluate import _check, head_modes

GMM_MODES = 3                                                                    # nr_max_modes 4 fits 1 .. 3 modes


class PredictResult(object):
    """Per-image NumPy arrays in dataset.image_ids order: image_ids, loc_est [N,3], q_est [N,4] ([x, y, z, w]) and the confidence
    the heads give without a truth to compare with: loc_peak (location classification: the largest softmax probability of the
    location bins), ori_peak and ori_lambda (soft classification: the largest probability of the orientation bins, and the largest
    eigenvalue of the PMF's scatter matrix sum_i w_i q_i q_i^T -- 1 for a point mass, 1/4 for a uniform spread); None where the
    head does not define them.  With multimodal: modes [N,3,4], mode_priors [N,3] (descending; unused slots 0) and n_modes [N]."""

    def __init__(self, image_ids, table, loc_class, soft, gmm=None):
        from . import hip
        t = np.asarray(table, dtype=np.float64)
        self.image_ids = np.asarray(image_ids)
        self.loc_est = t[:, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3].copy()
        self.q_est = t[:, hip.DEC_Q_EST:hip.DEC_Q_EST + 4].copy()
        self.loc_peak = t[:, hip.DEC_LOC_PEAK].copy() if loc_class else None
        self.ori_peak = t[:, hip.DEC_ORI_PEAK].copy() if soft else None
        self.ori_lambda = t[:, hip.DEC_ORI_LAMBDA].copy() if soft else None
        self.modes, self.mode_priors, self.n_modes = gmm if gmm is not None else (None, None, None)


def predict(model, dataset, multimodal=False, workers=None, cache=None):
    """Pose estimates of every image of `dataset` -> PredictResult.  The dataset needs image_ids, load_image, image_info and, for
    the classification heads, histogram_3D_map / ori_histogram_map; no label loader is called.  multimodal=True (soft
    classification only) also fits up to three orientation modes per image (urso_quat_gmm_fit: var = (BETA / ORI_BINS_PER_DIM)^2 /
    12, 5 iterations, nr_max_modes 4) and returns them; without a truth to pick a mode by, q_est stays the soft-argmax estimate.  cache: as in evaluate() -- a
    frame_cache.FrameCache of the caller's that keeps the raw frames on the device between calls (Config.DEVICE_RESIZE only)."""
    soft = _check(model, dataset, multimodal, "predict")
    import torch
    from . import hip
    from .feeder import EvalFeeder
    cfg, eng = model.config, model._engine
    loc_mode, ori_mode = head_modes(cfg)
    loc_class = loc_mode == hip.EVAL_LOC_CLASS
    ids = list(dataset.image_ids)
    N, B, dev = len(ids), eng.B, eng.device
    table = torch.full((max(N, 1), hip.DEC_COLS), float("nan"), dtype=torch.float64, device=dev)
    loc_map = torch.as_tensor(np.asarray(dataset.histogram_3D_map, dtype=np.float64)).to(dev).contiguous() if loc_class else None
    hq = q_soft = scatter = mean = prior = nm = None
    if soft:
        hq = torch.as_tensor(np.ascontiguousarray(dataset.ori_histogram_map, dtype=np.float32)).to(dev).contiguous()
        q_soft = torch.empty(B, 4, dtype=torch.float32, device=dev)
        scatter = torch.empty(B, 16, dtype=torch.float32, device=dev)
        if multimodal:                                                           # whole-dataset outputs: each batch fits into its rows
            rows = max(N, 1)
            mean = torch.zeros(rows, GMM_MODES, 4, dtype=torch.float32, device=dev)
            gv, prior, gs = (torch.zeros(rows, GMM_MODES, dtype=torch.float32, device=dev) for _ in range(3))
            nm = torch.zeros(rows, dtype=torch.int32, device=dev)
            var = (cfg.BETA / cfg.ORI_BINS_PER_DIM) ** 2 / 12
    if workers is None:
        workers = int(getattr(cfg, "LOADER_WORKERS", min(8, os.cpu_count() or 1)))
    feed = EvalFeeder(model, dataset, cfg, workers=workers, labels=False, cache=cache)
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
            n, r0 = bt.n, bt.row0
            z = None
            if soft:
                z = ori[:n].contiguous()
                hip.quat_wavg_decode(n, z.shape[1], z, hq, q_soft, scatter)
                if multimodal:
                    hip.quat_gmm_fit(n, z.shape[1], z, False, hq, var, 5, 4, mean[r0:r0 + n], gv[r0:r0 + n], prior[r0:r0 + n],
                                     gs[r0:r0 + n], nm[r0:r0 + n])
                ori = q_soft
            hip.pose_decode(B, n, r0, loc_mode, ori_mode, loc, ori, table, ori2=ori2, loc_map=loc_map, ori_logits=z,
                            ori_map_rows=hq.shape[0] if soft else 0, ori_scatter=scatter)
    finally:
        feed.close()
    host = table[:N].cpu().numpy()                                               # the one read of the table
    gmm = (mean[:N].cpu().numpy(), prior[:N].cpu().numpy(), nm[:N].cpu().numpy()) if multimodal else None
    return PredictResult(ids, host, loc_class, soft, gmm)
