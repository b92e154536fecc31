"""Ensemble inference: predict() / evaluate() / test_and_submit() with members=[...], the Bayesian model average of 1 .. 64 weight sets
of one network.

WEIGHT_EMA, SWA and swag_weights + save_weights all write several weight sets for one network.  For a classification head the model
average is the mean of the members' PMFs, decoded once -- it is not a mean of decoded poses, and the member PMFs never leave the device.
The pass below runs the one inference pass of ursonet_amd/infer.py once per member over the dataset (members outer, dataset inner: a
weight load is the expensive step), adds each member's bin probabilities into fp64 accumulators on the device (urso_ens_add), and
closes with, per chunk of B rows: one urso_pose_fuse_views over the members' decoded rows (identity rotations: the fused pose of the
regression heads, and for every head how far the members' poses spread), and for each classification head urso_ens_settle, whose
log-probabilities the existing decode kernels take in the place of logits.  Per image and classification head the result carries the
predictive entropy H[mean_j p_j], the mean member entropy mean_j H[p_j] and their difference, the mutual information between the
prediction and the member (BALD): the epistemic part of the uncertainty.

add64 / settle64 are the two kernels in NumPy float64, the written specification (include/ursonet_train.h has the reduction order of the
device, which they do not reproduce: tests bound the difference by the operation count).  Nothing here needs torch, the engine or the
library before Members and the size check have passed.
"""
import os

import numpy as np

MAX_MEMBERS = 64                   # URSO_ENS_MAX_MEMBERS (include/ursonet_train.h)
STAT, COLS = 4, 8                  # URSO_ENS_STAT, URSO_ENS_COLS
H_MEAN, H_MEMBERS, MI, PEAK, ARGMAX, N_MEMBERS = range(6)      # URSO_ENS_* columns
FLT_MAX = np.float32(3.4028234663852886e38)


# ------------------------------------------------------------------ the two kernels in NumPy float64
def add64(logits, acc=None, stat=None):
    """urso_ens_add on fp32 logits [n, K]: -> (acc, stat) with the rows' softmax added to acc [n, K] and {H, 1, 0, 0} to stat [n, 4]
    (both None: the first member, which overwrites).  The inputs are not changed."""
    z = np.asarray(logits, dtype=np.float32)
    assert z.ndim == 2 and z.shape[1] >= 1 and (acc is None) == (stat is None)
    with np.errstate(all="ignore"):
        m = z.max(axis=1).astype(np.float64)                      # NaN-propagating
        d = z.astype(np.float64) - m[:, None]
        e = np.exp(d)
        Z = e.sum(axis=1)
        S = np.where(e == 0, 0.0, e * -d).sum(axis=1)             # a vanished term adds exactly 0, also for d = -inf
        p = e / Z[:, None]
        H = np.log(Z) + S / Z
    one = np.stack([H, np.ones_like(H), np.zeros_like(H), np.zeros_like(H)], axis=1)
    if acc is None:
        return p, one
    a, s = np.asarray(acc, dtype=np.float64) + p, np.array(stat, dtype=np.float64)
    s[:, 0] += H
    s[:, 1] += 1
    return a, s


def settle64(acc, stat, M):
    """urso_ens_settle on acc [n, K], stat [n, 4] over M members: -> (logp fp32 [n, K], table fp64 [n, COLS])."""
    acc, stat = np.asarray(acc, dtype=np.float64), np.asarray(stat, dtype=np.float64)
    if not 1 <= int(M) <= MAX_MEMBERS:
        raise ValueError("settle64: need 1 <= M <= %d (got %r)" % (MAX_MEMBERS, M))
    with np.errstate(all="ignore"):
        p = acc / float(M)
        lg = np.log(p)
        logp = np.where(p == 0, -FLT_MAX, lg.astype(np.float32)).astype(np.float32)
        hbar = -np.where(p == 0, 0.0, p * lg).sum(axis=1)
        hmem = stat[:, 0] / float(M)
        diff = hbar - hmem
    t = np.zeros((acc.shape[0], COLS))
    t[:, H_MEAN], t[:, H_MEMBERS] = hbar, hmem
    t[:, MI] = np.where(diff < 0, 0.0, diff)                      # a NaN stays
    t[:, PEAK] = p.max(axis=1)                                    # NaN-propagating; argmax: the first NaN, else the lowest index of the peak
    t[:, ARGMAX] = p.argmax(axis=1)
    t[:, N_MEMBERS] = stat[:, 1]
    return logp, t


# ------------------------------------------------------------------ the member list
class Members(object):
    """The validated member list of one call: 1 .. 64 entries, each the path of a .h5 / .npz weights file (net.read_weights_file) or a
    {layer: {weight: array}} dict.  ValueError (no GPU needed): not a list or tuple, an empty one, more than 64 entries, an entry of
    another type, a file that does not exist, views together with members."""

    def __init__(self, members, views=None, who="predict"):
        if views is not None:
            raise ValueError("%s(members=...) cannot be combined with views=...: run the view fusion per member file instead" % who)
        if isinstance(members, (str, bytes, dict)) or not isinstance(members, (list, tuple)):
            raise ValueError("%s: members must be a list of weights files (.h5 / .npz) or {layer: {weight: array}} dicts, got %s"
                             % (who, type(members).__name__))
        if not 1 <= len(members) <= MAX_MEMBERS:
            raise ValueError("%s: members needs 1 .. %d weight sets (got %d)" % (who, MAX_MEMBERS, len(members)))
        for j, m in enumerate(members):
            if isinstance(m, dict):
                if not m or not all(isinstance(ws, dict) for ws in m.values()):
                    raise ValueError("%s: member %d must map layer names to {weight: array} dicts" % (who, j))
            elif isinstance(m, (str, os.PathLike)):
                p = os.fspath(m)
                if not (p.endswith(".h5") or p.endswith(".npz")):
                    raise ValueError("%s: member %d must be a .h5 or .npz weights file (got %r)" % (who, j, p))
                if not os.path.isfile(p):
                    raise ValueError("%s: member %d: no such weights file %r" % (who, j, p))
            else:
                raise ValueError("%s: member %d must be a weights file path or a {layer: {weight: array}} dict, got %s"
                                 % (who, j, type(m).__name__))
        self.entries, self.who = list(members), who

    def __len__(self):
        return len(self.entries)

    def load(self, j, layers):
        """Member j as {layer: {weight: array}} restricted to `layers` (the graph's).  ValueError: a layer of the graph that the member
        lacks -- an average over networks that differ in anything but the listed weights is not a model average."""
        m = self.entries[j]
        if not isinstance(m, dict):
            from .net import read_weights_file
            m = read_weights_file(os.fspath(m))
        missing = [ln for ln in layers if ln not in m]
        if missing:
            raise ValueError("%s: member %d lacks %d layer(s) of the network: %s" % (self.who, j, len(missing), missing[:5]))
        return dict((ln, m[ln]) for ln in layers)


def accumulator_bytes(N, M, k_ori, k_loc, truth, dec_cols=12):
    """Device bytes of the whole-dataset buffers of the pass for N images and M members: the fp64 PMF accumulators [N, K] of each
    classification head with their stat and uncertainty rows, the members' decoded rows [M * N, DEC_COLS] and, with a truth, the
    poses and the stored encoded targets (fp32 [N, K])."""
    per_head = lambda k: (N * (k * 8 + (STAT + COLS) * 8 + (k * 4 if truth else 0))) if k else 0      # noqa: E731
    return per_head(k_ori) + per_head(k_loc) + M * N * dec_cols * 8 + (N * 7 * 8 if truth else 0)


def check_size(N, M, k_ori, k_loc, truth, max_gb, who="predict"):
    """ValueError, naming the figure, when the pass would hold more than max_gb GiB on the device."""
    try:
        limit = float(max_gb)
    except (TypeError, ValueError):
        limit = float("nan")
    if not limit > 0:
        raise ValueError("%s: max_gb must be a number > 0 (got %r)" % (who, max_gb))
    need = accumulator_bytes(N, M, k_ori, k_loc, truth)
    if need > limit * 2 ** 30:
        raise ValueError("%s(members=...): the accumulators of %d images (%d orientation and %d location bins in fp64, %d members' rows) "
                         "need %.3f GiB on the device, more than max_gb = %g; predict the dataset in parts or raise max_gb"
                         % (who, N, k_ori, k_loc, M, need / 2.0 ** 30, limit))
    return need


def head_bins(model):
    """(K_ori, K_loc): the bins of the classification heads of the model's graph, 0 for a regression head."""
    cfg, outs = model.config, model._engine.graph.outputs
    soft = not (cfg.REGRESS_ORI or cfg.REGRESS_KEYPOINTS)
    return (int(outs["ori"].c) if soft else 0), (0 if cfg.REGRESS_LOC else int(outs["loc"].c))


# ------------------------------------------------------------------ the result
class EnsembleTables(object):
    """What the pass read back, as NumPy fp64: M, fuse [N, FUSE_COLS], head (the DEC or EVAL table of the averaged PMFs' decode, None
    without a classification head), ens_ori / ens_loc [N, COLS] (None for a regression head), gmm (mean, prior, n_modes) or None,
    loc_gt [N, 3] or None."""

    def __init__(self, M, fuse, head, ens_ori, ens_loc, gmm, loc_gt):
        self.M, self.fuse, self.head, self.ens_ori, self.ens_loc, self.gmm, self.loc_gt = M, fuse, head, ens_ori, ens_loc, gmm, loc_gt


def no_member_fields(res):
    """The fields of a PredictResult / EvalResult that only an ensemble defines, all None."""
    res.n_members = res.member_loc_spread = res.member_ori_spread = res.member_lambda = None
    res.ori_entropy = res.ori_member_entropy = res.ori_mi = res.loc_entropy = res.loc_member_entropy = res.loc_mi = None


def member_fields(res, out):
    """The ensemble's own fields on `res` from EnsembleTables: the members' disagreement (urso_pose_fuse_views' columns) and, per
    classification head, the three entropies in nats."""
    from . import hip
    f = out.fuse
    res.n_members = int(out.M)
    res.member_loc_spread, res.member_ori_spread = f[:, hip.FUSE_LOC_SPREAD].copy(), f[:, hip.FUSE_ORI_SPREAD].copy()
    res.member_lambda = f[:, hip.FUSE_VIEW_LAMBDA].copy()
    for name, t in (("ori", out.ens_ori), ("loc", out.ens_loc)):
        cols = (None, None, None) if t is None else (t[:, H_MEAN].copy(), t[:, H_MEMBERS].copy(), t[:, MI].copy())
        for key, v in zip(("entropy", "member_entropy", "mi"), cols):
            setattr(res, "%s_%s" % (name, key), v)


def predict_fields(res, out, loc_class, soft):
    """A PredictResult's fields from EnsembleTables: the fused pose, with each classification head's estimate and confidence taken from
    the decode of its averaged PMF."""
    from . import hip
    from .infer import fuse_columns
    fuse_columns(res, out.fuse, False)
    res.loc_spread = res.ori_spread = res.view_lambda = res.n_views = None
    res.loc_peak = res.ori_peak = res.ori_lambda = None
    if out.head is not None:
        h = out.head
        if loc_class:
            res.loc_est, res.loc_peak = h[:, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3].copy(), h[:, hip.DEC_LOC_PEAK].copy()
        if soft:
            res.q_est = h[:, hip.DEC_Q_EST:hip.DEC_Q_EST + 4].copy()
            res.ori_peak, res.ori_lambda = h[:, hip.DEC_ORI_PEAK].copy(), h[:, hip.DEC_ORI_LAMBDA].copy()
    member_fields(res, out)


def eval_fields(res, out, loc_class, soft, multimodal):
    """An EvalResult's fields from EnsembleTables: the fused pose and its errors, with each classification head's estimate and errors
    taken from urso_pose_eval on its averaged PMF; with one head of each kind ESA is put together from the two by the kernel's formula."""
    from . import hip
    from .infer import fuse_columns
    fuse_columns(res, out.fuse, True)
    res.loc_spread = res.ori_spread = res.view_lambda = res.n_views = None
    res.loc_encoded_err = res.ori_encoded_err = res.ori_err_soft = res.mode = None
    if out.head is not None:
        h = out.head
        if loc_class:
            res.loc_est, res.loc_err = h[:, hip.EVAL_LOC_EST:hip.EVAL_LOC_EST + 3].copy(), h[:, hip.EVAL_LOC_ERR].copy()
            res.loc_encoded_err = h[:, hip.EVAL_LOC_ENC_ERR].copy()
        if soft:
            res.q_est, res.ori_err = h[:, hip.EVAL_Q_EST:hip.EVAL_Q_EST + 4].copy(), h[:, hip.EVAL_ORI_ERR].copy()
            res.ori_encoded_err = h[:, hip.EVAL_ORI_ENC_ERR].copy()
            if multimodal:
                res.ori_err_soft, res.mode = h[:, hip.EVAL_ORI_ERR_SOFT].copy(), h[:, hip.EVAL_MODE].astype(np.int32)
        if loc_class and soft:
            res.esa = h[:, hip.EVAL_ESA].copy()
        else:                                                     # ESA = LOC_ERR / ||loc_gt|| + the orientation error in radians
            res.esa = res.loc_err / np.sqrt((out.loc_gt ** 2).sum(axis=1)) + res.ori_err * np.pi / 180
    member_fields(res, out)


# ------------------------------------------------------------------ the pass
class EnsemblePass(object):
    """One call's ensemble pass.  truth: evaluate() (labels are loaded with the first member and kept on the device for the closing
    pass); else predict().  run() -> (EnsembleTables, the first feeder's loc_dtype)."""

    def __init__(self, model, dataset, members, multimodal=False, truth=False, who="predict", workers=None, cache=None, max_gb=16):
        from .infer import PosePass, check_heads, loader_workers
        assert isinstance(members, Members)
        check_heads(model, dataset, multimodal, who)
        self.model, self.dataset, self.members, self.multimodal, self.truth, self.who = model, dataset, members, multimodal, truth, who
        self.ids = list(dataset.image_ids)
        self.N, self.M = len(self.ids), len(members)
        self.k_ori, self.k_loc = head_bins(model)
        check_size(self.N, self.M, self.k_ori, self.k_loc, truth, max_gb, who)       # before any GPU work
        self.ps = PosePass(model, dataset, multimodal, scatter=True, who=who)
        self.workers, self.cache = loader_workers(self.ps.cfg, workers), cache

    def run(self):
        eng, layers = self.model._engine, list(self.model._graph.params)
        saved = eng.get_weights()
        try:
            return self._run(eng, layers)
        finally:
            eng.set_weights(saved, strict=True)

    def _run(self, eng, layers):
        from .feeder import EvalFeeder
        from .infer import GMM_ITERATIONS, GMM_MAX_MODES
        ps, hip, torch = self.ps, self.ps.hip, self.ps.torch
        N, M, B, dev = self.N, self.M, self.ps.B, self.ps.dev
        rows = max(N, 1) + B                                       # a chunk's kernels index B rows from its first: B spare rows behind the last
        f64 = dict(dtype=torch.float64, device=dev)
        member_table = ps.table(M * max(N, 1) + B, hip.DEC_COLS)   # member j's rows at [j * N, j * N + N)
        acc_ori = stat_ori = acc_loc = stat_loc = None
        if ps.soft:
            acc_ori, stat_ori = torch.empty(max(N, 1), self.k_ori, **f64), torch.empty(max(N, 1), hip.ENS_STAT, **f64)
        if ps.loc_class:
            acc_loc, stat_loc = torch.empty(max(N, 1), self.k_loc, **f64), torch.empty(max(N, 1), hip.ENS_STAT, **f64)
        gt_loc = gt_q = enc_loc = enc_ori = None
        if self.truth:
            gt_loc, gt_q = ps.table(rows, 3), ps.table(rows, 4)
            enc_loc = torch.zeros(rows, self.k_loc, dtype=torch.float32, device=dev) if ps.loc_class else None
            enc_ori = torch.zeros(rows, self.k_ori, dtype=torch.float32, device=dev) if ps.soft else None
        loc_dtype = None

        # members outer, dataset inner
        for j in range(M):
            eng.set_weights(self.members.load(j, layers), strict=False)
            labels = self.truth and j == 0
            feed = EvalFeeder(self.model, self.dataset, ps.cfg, enc_loc=labels and ps.loc_class, enc_ori=labels and ps.soft,
                              workers=self.workers, labels=labels, cache=self.cache)
            try:
                for bt in feed:
                    ps.run(bt.images)
                    heads = ps.heads(bt.n)
                    ps.decode_into(member_table, bt.n, j * N + bt.row0, heads)
                    loc, _ori, _ori2, z = heads
                    if ps.soft:
                        hip.ens_add(bt.n, bt.n, bt.row0, z, acc_ori, stat_ori, j == 0)
                    if ps.loc_class:
                        hip.ens_add(B, bt.n, bt.row0, loc, acc_loc, stat_loc, j == 0)
                    if labels:                                     # the staging buffers are the feeder's: the truth moves to rows of its own
                        sl = slice(bt.row0, bt.row0 + bt.n)
                        gt_loc[sl].copy_(bt.loc_gt[:bt.n]); gt_q[sl].copy_(bt.q_gt[:bt.n])
                        if enc_loc is not None:
                            enc_loc[sl].copy_(bt.enc_loc[:bt.n])
                        if enc_ori is not None:
                            enc_ori[sl].copy_(bt.enc_ori[:bt.n])
            finally:
                feed.close()
            if labels:
                loc_dtype = feed.loc_dtype

        # the closing pass, per chunk of B rows
        ident = torch.eye(3, **f64).reshape(1, 9).repeat(M, 1).contiguous()
        qr = torch.tensor([[0.0, 0.0, 0.0, 1.0]], **f64).repeat(M, 1).contiguous()
        fuse = ps.table(max(N, 1), hip.FUSE_COLS)
        any_class = ps.soft or ps.loc_class
        head = ps.table(max(N, 1), hip.EVAL_COLS if self.truth else hip.DEC_COLS) if any_class else None
        ens_ori = ps.table(max(N, 1), hip.ENS_COLS) if ps.soft else None
        ens_loc = ps.table(max(N, 1), hip.ENS_COLS) if ps.loc_class else None
        logp_ori = torch.empty(B, self.k_ori, dtype=torch.float32, device=dev) if ps.soft else None
        logp_loc = torch.empty(B, self.k_loc, dtype=torch.float32, device=dev) if ps.loc_class else None
        zeros_loc = torch.zeros(B, 3, dtype=torch.float32, device=dev)                      # stand-ins for a regression head beside a
        unit_q = torch.tensor([[0.0, 0.0, 0.0, 1.0]], dtype=torch.float32, device=dev).repeat(B, 1).contiguous()   # classification head
        gmm = None
        if self.multimodal:                                        # predict: whole-dataset outputs; evaluate: the chunk's (urso_pose_eval indexes by batch row)
            gmm = ps.gmm_buffers(B) if self.truth else ps.gmm_buffers(max(N, 1), zeroed=True)
        for row0 in range(0, N, B):
            n = min(B, N - row0)
            tl, tq = (gt_loc[row0:row0 + B], gt_q[row0:row0 + B]) if self.truth else (None, None)
            hip.pose_fuse_views(B, n, row0, member_table[row0:], ident, qr, fuse, loc_gt=tl, q_gt=tq, est_view_rows=max(N, 1))
            if not any_class:
                continue
            loc, loc_mode, ori, ori_mode, z, chunk_gmm = zeros_loc, hip.EVAL_LOC_REGRESS, unit_q, hip.EVAL_ORI_QUAT, None, None
            if ps.loc_class:
                hip.ens_settle(n, row0, M, acc_loc, stat_loc, logp_loc, ens_loc)
                loc, loc_mode = logp_loc, hip.EVAL_LOC_CLASS
            if ps.soft:
                hip.ens_settle(n, row0, M, acc_ori, stat_ori, logp_ori, ens_ori)
                z = logp_ori[:n]
                hip.quat_wavg_decode(n, self.k_ori, z, ps.hq, ps.q_soft, ps.scatter)
                if gmm is not None:
                    chunk_gmm = gmm if self.truth else [t[row0:row0 + n] for t in gmm]
                    hip.quat_gmm_fit(n, self.k_ori, z, False, ps.hq, ps.var, GMM_ITERATIONS, GMM_MAX_MODES, *chunk_gmm)
                ori, ori_mode = ps.q_soft, hip.EVAL_ORI_SOFT
            if self.truth:
                hip.pose_eval(B, n, row0, loc_mode, ori_mode, loc, ori, tl, tq, head, loc_map=ps.loc_map if ps.loc_class else None,
                              ori_map=ps.hq if ps.soft else None, enc_loc=enc_loc[row0:row0 + B] if ps.loc_class else None,
                              enc_ori=enc_ori[row0:row0 + B] if ps.soft else None,
                              gmm_mean=chunk_gmm[0] if chunk_gmm else None, gmm_nmodes=chunk_gmm[4] if chunk_gmm else None)
            else:
                hip.pose_decode(B, n, row0, loc_mode, ori_mode, loc, ori, head, loc_map=ps.loc_map if ps.loc_class else None, ori_logits=z,
                                ori_map_rows=ps.hq.shape[0] if ps.soft else 0, ori_scatter=ps.scatter if ps.soft else None)

        # the one read of the tables
        host = lambda t: None if t is None else t[:N].cpu().numpy()                          # noqa: E731
        fit = None
        if self.multimodal and not self.truth:
            fit = tuple(gmm[i][:N].cpu().numpy() for i in (0, 2, 4))                         # mean, prior, n_modes
        out = EnsembleTables(M, host(fuse), host(head), host(ens_ori), host(ens_loc), fit, host(gt_loc))
        for t in (out.ens_ori, out.ens_loc):
            if t is not None and not np.all(t[:, N_MEMBERS] == M):
                raise RuntimeError("%s(members=...): a row of the accumulators holds %s members, not %d" % (self.who, sorted(set(t[:, N_MEMBERS])), M))
        return out, loc_dtype

