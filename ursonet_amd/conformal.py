"""Split conformal prediction for the pose heads (Vovk et al., 2005; Papadopoulos et al., 2002): conformal() turns held-out labelled
data into per-head levels, predict() / evaluate() / test_and_submit() with conformal=... turn them into a per-image error bound with a
finite-sample coverage guarantee.

For a classification head the score of a labelled image is the PMF mass of the bins STRICTLY closer to the estimate than the truth is;
with q the k-th smallest of n calibration scores, k = ceil((n + 1)(1 - alpha)), a new image's truth is at least as close to its
estimate as v* -- the closest key at which the mass of the bins at least as close exceeds q -- with probability >= 1 - alpha, provided
calibration and test images are exchangeable.  The bound is value(v*): degrees for the orientation head (URSO_CONF_ANGLE), metres for
the location head (URSO_CONF_EUCLID).  The guarantee is marginal (over the draw of calibration set and image), not per image.  A
regression head has no PMF: its score is its error and its bound the constant quantile.

weights64 / score64 / bound64 are the two kernels (urso_conf_score / urso_conf_bound, include/ursonet_infer.h) in NumPy float64 and
unsigned 64-bit integers, the written specification.  The weights are integers, so every sum is exact whatever its order: the kernels'
results equal these bit for bit wherever exp does (both are documented to 1 ulp; a weight is rint(exp(d) 2^34), so they differ only where
exp(d) 2^34 lies within an ulp of a rounding boundary).  Nothing here needs torch, the engine or the library before every refusal of
conformal() has passed.
"""
import json
import math

import numpy as np

from .infer import Subset, refuse_launcher

SHIFT, MAX_K, COLS = 34, 1 << 18, 8                               # URSO_CONF_SHIFT, URSO_CONF_MAX_K, URSO_CONF_COLS (include/ursonet_infer.h)
ANGLE, EUCLID = 0, 1                                              # URSO_CONF_ANGLE, URSO_CONF_EUCLID
SCORE, C_MASS, W_SUM, KEY_REF, ERR, NEAR = range(6)               # the score row
BOUND, KEY, MASS, COUNT, BOUND_W = range(5)                       # the bound row
_FLIP = np.uint64(0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------ the two kernels in NumPy
def weights64(z):
    """The integer weights of fp32 logit rows z [n, K]: -> (w uint64 [n, K], W uint64 [n], ok bool [n]); ok: the row's maximum is finite
    (the weights of any other row mean nothing)."""
    z = np.asarray(z, dtype=np.float32)
    assert z.ndim == 2 and 1 <= z.shape[1] <= MAX_K
    with np.errstate(all="ignore"):
        m = z.max(axis=1)                                         # NaN-propagating
        ok = np.isfinite(m)
        d = z.astype(np.float64) - np.where(ok, m, 0).astype(np.float64)[:, None]
        s = np.exp(d) * float(2 ** SHIFT)
        w = np.rint(np.where(np.isfinite(s), s, 0.0)).astype(np.uint64)
    return w, w.sum(axis=1, dtype=np.uint64), ok


def _key(metric, e, h):
    """The key from lists of broadcastable fp64 components of the estimate e and of the point h, in the header's operation order."""
    with np.errstate(all="ignore"):
        if metric == ANGLE:
            s = ((e[0] * h[0] + e[1] * h[1]) + e[2] * h[2]) + e[3] * h[3]
            a = np.abs(s)
            return np.where(a > 1.0, 1.0, a)
        assert metric == EUCLID
        d = [h[j] - e[j] for j in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def keys64(metric, bin_map, est):
    """The keys [n, K] of the bins of bin_map (ANGLE: fp32 [K, 4]; EUCLID: fp64 [K, 3]) around the estimates est fp64 [n, 4 | 3]."""
    D = 4 if metric == ANGLE else 3
    h = np.asarray(bin_map, dtype=np.float32 if metric == ANGLE else np.float64).astype(np.float64)
    e = np.asarray(est, dtype=np.float64)
    assert h.ndim == 2 and h.shape[1] == D and e.ndim == 2 and e.shape[1] == D
    return _key(metric, [e[:, j:j + 1] for j in range(D)], [h[None, :, j] for j in range(D)])


def ref_keys64(metric, est, ref):
    """key_ref [n]: the key of the truth ref fp64 [n, 4 | 3] around est [n, 4 | 3], the truth in the place of the map entry."""
    D = 4 if metric == ANGLE else 3
    e, r = np.asarray(est, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert e.shape == r.shape and e.ndim == 2 and e.shape[1] == D
    return _key(metric, [e[:, j] for j in range(D)], [r[:, j] for j in range(D)])


def ranks(metric, key):
    """The rank of a key: its bit pattern as uint64, complemented for ANGLE, so that a smaller rank is closer under either metric."""
    b = np.ascontiguousarray(key, dtype=np.float64).view(np.uint64)
    return b ^ _FLIP if metric == ANGLE else b


def value(metric, key):
    """The error a key stands for: degrees (ANGLE) or metres (EUCLID)."""
    key = np.asarray(key, dtype=np.float64)
    with np.errstate(all="ignore"):
        return ((2.0 * np.arccos(key)) * 180.0) / np.pi if metric == ANGLE else np.sqrt(key)


def _finite_rows(ok, *tables):
    for t in tables:
        ok = ok & np.all(np.isfinite(np.asarray(t, dtype=np.float64)), axis=1)
    return ok


def score64(z, bin_map, est, ref, metric):
    """urso_conf_score: -> fp64 [n, 8] = {SCORE, C, W, KEY_REF, ERR, NEAR, 0, 0}; a row that is not finite is NaN throughout."""
    w, W, ok = weights64(z)
    ok = _finite_rows(ok, est, ref)
    key_ref = ref_keys64(metric, est, ref)
    near = ranks(metric, keys64(metric, bin_map, est)) < ranks(metric, key_ref)[:, None]
    Cm = np.where(near, w, np.uint64(0)).sum(axis=1, dtype=np.uint64)
    out = np.zeros((w.shape[0], COLS))
    with np.errstate(all="ignore"):
        out[:, SCORE] = Cm.astype(np.float64) / W.astype(np.float64)
    out[:, C_MASS], out[:, W_SUM], out[:, KEY_REF] = Cm, W, key_ref
    out[:, ERR], out[:, NEAR] = value(metric, key_ref), near.sum(axis=1)
    out[~ok] = np.nan
    return out


def bound64(z, bin_map, est, metric, q):
    """urso_conf_bound at the level q (> 0, +inf allowed): -> fp64 [n, 8] = {BOUND, KEY, MASS, COUNT, W, 0, 0, 0}."""
    q = float(q)
    assert q > 0
    w, W, ok = weights64(z)
    ok = _finite_rows(ok, est)
    r = ranks(metric, keys64(metric, bin_map, est))
    n, K = w.shape
    out = np.zeros((n, COLS))
    for b in range(n):
        if not ok[b]:
            out[b] = np.nan
            continue
        order = np.argsort(r[b], kind="stable")
        rs, G = r[b][order], np.cumsum(w[b][order], dtype=np.uint64)
        last = np.flatnonzero(np.append(rs[1:] != rs[:-1], True))               # the last bin of every group of equal keys
        Wd = float(W[b])
        hit = np.flatnonzero(G[last].astype(np.float64) / Wd > q)
        if len(hit) == 0:
            out[b, :5] = (180.0 if metric == ANGLE else np.inf), np.nan, 1.0, K, Wd
            continue
        i = last[hit[0]]
        key = (rs[i:i + 1] ^ _FLIP if metric == ANGLE else rs[i:i + 1]).view(np.float64)[0]
        out[b, :5] = value(metric, key), key, float(G[i]) / Wd, i + 1, Wd
    return out


def quantile(scores, alpha):
    """The conformal level: the k-th smallest score, k = ceil((n + 1)(1 - alpha)); +inf where k > n (too few scores for this alpha)."""
    s = np.sort(np.asarray(scores, dtype=np.float64).reshape(-1))
    n = len(s)
    k = int(math.ceil((n + 1) * (1.0 - float(alpha))))
    return float("inf") if k > n or n == 0 else float(s[max(k, 1) - 1])


# ------------------------------------------------------------------ the result
def _alpha(alpha, who="conformal"):
    try:
        f = float(alpha)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(alpha, bool) or not (0 < f < 1):
        raise ValueError("%s: alpha must be a number in (0, 1) (got %r)" % (who, alpha))
    return f


class Conformal(object):
    """The conformal levels of a model's heads: alpha, per head the kind (ori_kind / loc_kind: "pmf" for a classification head, whose
    scores are PMF masses and whose bound varies per image, "error" for a regression head, whose scores are errors -- degrees / metres --
    and whose bound is the constant level), the sorted calibration scores (ori_scores / loc_scores), the level ori_q / loc_q (quantile()
    of the scores at alpha), k_ori / k_loc (the heads' bin counts, 0 for a regression head), n_images, and ori_beta / loc_beta: the inverse
    temperatures of the calibration it was fitted under (None: none) -- it applies only under the same ones.  at(alpha) gives the levels
    for another alpha from the kept scores, without a GPU.  save(path) / Conformal.load(path): JSON, floats by repr, bit for bit."""

    def __init__(self, alpha, ori_kind, loc_kind, ori_scores, loc_scores, k_ori=0, k_loc=0, n_images=None, ori_beta=None, loc_beta=None,
                 ori_q=None, loc_q=None):
        self.alpha = _alpha(alpha, "Conformal")
        for kind in (ori_kind, loc_kind):
            if kind not in ("pmf", "error"):
                raise ValueError("Conformal: a head's kind is 'pmf' or 'error' (got %r)" % (kind,))
        self.ori_kind, self.loc_kind = ori_kind, loc_kind
        self.ori_scores, self.loc_scores = (sorted(float(x) for x in s) for s in (ori_scores, loc_scores))
        self.k_ori, self.k_loc = int(k_ori or 0), int(k_loc or 0)
        self.n_images = len(self.ori_scores) if n_images is None else int(n_images)
        self.ori_beta, self.loc_beta = (None if b is None else float(b) for b in (ori_beta, loc_beta))
        self.ori_q, self.loc_q = quantile(self.ori_scores, self.alpha), quantile(self.loc_scores, self.alpha)
        for name, given, mine in (("ori_q", ori_q, self.ori_q), ("loc_q", loc_q, self.loc_q)):
            if given is not None and float(given) != mine:
                raise ValueError("Conformal: %s = %r is not the level of the scores at alpha = %r (%r)" % (name, given, self.alpha, mine))

    def at(self, alpha):
        """The same scores at another alpha."""
        d = self.to_dict()
        d.update(alpha=alpha, ori_q=None, loc_q=None)
        return Conformal(**d)

    def to_dict(self):
        return dict(alpha=self.alpha, ori_kind=self.ori_kind, loc_kind=self.loc_kind, ori_scores=self.ori_scores, loc_scores=self.loc_scores,
                    k_ori=self.k_ori, k_loc=self.k_loc, n_images=self.n_images, ori_beta=self.ori_beta, loc_beta=self.loc_beta,
                    ori_q=self.ori_q, loc_q=self.loc_q)

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_dict(), f, indent=1, sort_keys=True)
            f.write("\n")
        return path

    @classmethod
    def load(cls, path):
        with open(path) as f:
            return cls(**json.load(f))

    def __eq__(self, other):
        return isinstance(other, Conformal) and self.to_dict() == other.to_dict()

    def __repr__(self):
        d = self.to_dict()
        d["ori_scores"], d["loc_scores"] = "<%d>" % len(self.ori_scores), "<%d>" % len(self.loc_scores)
        return "Conformal(%s)" % ", ".join("%s=%s" % kv for kv in sorted(d.items()) if kv[1] is not None)

    def line(self, res=None):
        """The line evaluate(conformal=...) prints behind its usual ones: the target and, given the result, per head the empirical coverage
        and the mean / median bound."""
        parts = []
        for name, unit, head in (("orientation", "deg", "ori"), ("location", "m", "loc")):
            txt = "%s level %s (%s)" % (name, getattr(self, head + "_q"), getattr(self, head + "_kind"))
            if res is not None:
                cov, bound = getattr(res, head + "_covered"), getattr(res, head + "_bound")
                txt = "%s coverage %s, bound mean %s median %s %s, level %s (%s)" % (
                    name, np.mean(cov), np.mean(bound), np.median(bound), unit, getattr(self, head + "_q"), getattr(self, head + "_kind"))
            parts.append(txt)
        return "Conformal: target coverage %s on %d calibration images; %s" % (1.0 - self.alpha, self.n_images, "; ".join(parts))

    def check_calibration(self, calibration, who="predict"):
        """ValueError where the calibration applied now is not the one the levels were fitted under: the scores are masses of another PMF."""
        now = (None, None) if calibration is None else (calibration.ori_beta, calibration.loc_beta)
        if now != (self.ori_beta, self.loc_beta):
            raise ValueError("%s: the conformal levels were fitted under the calibration betas (ori %r, loc %r), but calibration= gives "
                             "(ori %r, loc %r): scores and bounds must come from the same PMFs; run conformal() under this calibration"
                             % (who, self.ori_beta, self.loc_beta, now[0], now[1]))

    def check_model(self, k_ori, k_loc, who="predict"):
        """ValueError where the levels do not fit a model whose classification heads have k_ori / k_loc bins (0: a regression head)."""
        for name, mine, model in (("orientation", self.k_ori, k_ori), ("location", self.k_loc, k_loc)):
            if mine != model:
                said = lambda k: "%d bins" % k if k else "a regression output"      # noqa: E731
                raise ValueError("%s: the conformal levels were fitted on a model whose %s head has %s, this model's has %s"
                                 % (who, name, said(mine), said(model)))


def check_conformal(conformal, members=None, views=None, calibration=None, who="predict"):
    """The refusals of predict / evaluate / test_and_submit (conformal=...) that need neither the model nor a GPU."""
    if conformal is None:
        return None
    if not isinstance(conformal, Conformal):
        raise ValueError("%s: conformal must be a conformal.Conformal (from conformal() or Conformal.load()), got %s" % (who, type(conformal).__name__))
    if members is not None or views is not None:
        raise ValueError("%s: conformal=... cannot be combined with members=... or views=...: the levels were fitted on the plain pass of "
                         "one weight set" % who)
    conformal.check_calibration(calibration, who)
    return conformal


# ------------------------------------------------------------------ on the device
class ConformalPass(object):
    """The launches of one command on a PosePass ps: per classification head a fp64 device table [rows, 8] for the scores (labelled
    batches) and one for the bounds (levels given).  Nothing here synchronises; tables() reads once, at the end."""

    def __init__(self, ps, rows, levels=None, scores=False):
        hip, torch = ps.hip, ps.torch
        self.ps, self.hip = ps, hip
        self.heads = []                                             # (name, metric, est column, width, score table, bound table, q)
        for name, on, metric, col, D in (("ori", ps.soft, hip.CONF_ANGLE, hip.EVAL_Q_EST, 4), ("loc", ps.loc_class, hip.CONF_EUCLID, hip.EVAL_LOC_EST, 3)):
            if on:
                q = None if levels is None else getattr(levels, name + "_q")
                self.heads.append((name, metric, col, D, ps.table(rows, hip.CONF_COLS) if scores else None,
                                   ps.table(rows, hip.CONF_COLS) if q is not None else None, q))
        assert hip.EVAL_Q_EST == hip.DEC_Q_EST and hip.EVAL_LOC_EST == hip.DEC_LOC_EST
        hip.side_lib("infer")                                      # a missing library is an error here, not in the first batch
        self.torch = torch

    def launch(self, table, n, row0, heads, bt=None):
        """Behind eval_into / decode_into of rows [row0, row0 + n): est is read from the rows just written into `table`."""
        loc, _ori, _ori2, z = heads
        ps, hip = self.ps, self.hip
        for name, metric, col, D, scores, bounds, q in self.heads:
            logits, bin_map = (z, ps.hq) if name == "ori" else (loc, ps.loc_map)
            B = n if name == "ori" else ps.B                       # heads() hands the n valid rows of the orientation logits
            est = table[:, col:col + D]
            if scores is not None:
                hip.conf_score(B, n, row0, metric, logits, bin_map, est, bt.q_gt if name == "ori" else bt.loc_gt, scores)
            if bounds is not None:
                hip.conf_bound(B, n, row0, metric, q, logits, bin_map, est, bounds)

    def tables(self, N):
        """{head: (score table or None, bound table or None)} on the host, N rows."""
        return dict((h[0], tuple(None if t is None else t[:N].cpu().numpy() for t in h[4:6])) for h in self.heads)


def bound_fields(res, cf, tabs, N, truth=False):
    """Sets ori_bound / loc_bound, the region fields of the PMF heads and, with a truth, ori_covered / loc_covered on a result."""
    for head in ("ori", "loc"):
        kind, q = getattr(cf, head + "_kind"), getattr(cf, head + "_q")
        bins = mass = None
        if kind == "pmf":
            scores, bounds = tabs.get(head) or (np.zeros((0, COLS)), np.zeros((0, COLS)))   # (no batch ran: no image)
            bound, bins, mass = bounds[:, BOUND].copy(), bounds[:, COUNT].copy(), bounds[:, MASS].copy()
            covered = scores[:, SCORE] <= q if truth else None   # exactly: the truth's key is at least as close as the bound's
        else:
            bound = np.full(N, q)
            covered = getattr(res, head + "_err") <= q if truth else None
        setattr(res, head + "_bound", bound)
        setattr(res, head + "_region_bins", bins)
        setattr(res, head + "_region_mass", mass)
        if truth:
            setattr(res, head + "_covered", covered)


def no_bound_fields(res, truth=False):
    for head in ("ori", "loc"):
        for f in ("_bound", "_region_bins", "_region_mass") + (("_covered",) if truth else ()):
            setattr(res, head + f, None)


# ------------------------------------------------------------------ the fit over a dataset
def conformal(model, dataset, alpha=0.1, nr_images=None, workers=None, cache=None, calibration=None, *, members=None, views=None):
    """The conformal levels of every head of an inference model on a labelled dataset -> Conformal.  The dataset is walked once (the first
    nr_images of dataset.image_ids; None: all) with evaluate()'s feeder and inference pass; behind each batch's urso_pose_eval one
    urso_conf_score per classification head writes the images' scores into a device table that is read once at the end; a regression
    head's scores are its errors from the same EVAL table.  calibration: the calibrate.Calibration that will be applied with the levels
    (the scores are masses of the calibrated PMF).  The images must not be ones the model or the calibration was fitted on, and must be
    exchangeable with the images the bounds will be used on.  ValueError, before any GPU work: alpha outside (0, 1), a data-parallel
    launcher, members or views, no labelled image."""
    who = "conformal"
    alpha = _alpha(alpha, who)
    if members is not None or views is not None:
        raise ValueError("%s: members=... and views=... are not supported: the levels belong to the plain pass of one weight set" % who)
    refuse_launcher(model, who, "walk the whole dataset")
    from .calibrate import check_calibration
    check_calibration(calibration, None, who)
    ids = list(dataset.image_ids)
    if nr_images is not None:
        if int(nr_images) < 1:
            raise ValueError("%s: nr_images must be >= 1 or None (got %r)" % (who, nr_images))
        ids = ids[:int(nr_images)]
    N = len(ids)
    if N < 1:
        raise ValueError("%s: the dataset has no labelled images" % who)

    from .feeder import EvalFeeder
    from .infer import PosePass, loader_workers
    from .ensemble import head_bins
    ps = PosePass(model, dataset, False, who=who, calibration=calibration)
    hip = ps.hip
    k_ori, k_loc = head_bins(model)
    table = ps.table(N, hip.EVAL_COLS)
    cp = ConformalPass(ps, N, scores=True)
    feed = EvalFeeder(model, Subset(dataset, ids) if nr_images is not None else dataset, ps.cfg, enc_loc=ps.loc_class, enc_ori=ps.soft,
                      workers=loader_workers(ps.cfg, workers), cache=cache)
    try:
        for bt in feed:
            ps.run(bt.images)
            heads = ps.heads(bt.n)
            ps.eval_into(table, bt, heads)
            cp.launch(table, bt.n, bt.row0, heads, bt)
    finally:
        feed.close()
    host = table[:N].cpu().numpy()
    tabs = cp.tables(N)
    scores = {}
    for head, col in (("ori", hip.EVAL_ORI_ERR), ("loc", hip.EVAL_LOC_ERR)):
        s = tabs[head][0][:, SCORE] if head in tabs else host[:, col]
        if not np.all(np.isfinite(s)):
            raise ValueError("%s: %d of %d images have a score that is not finite (a NaN or infinite logit, estimate or truth) on the %s head"
                             % (who, int(np.sum(~np.isfinite(s))), N, "orientation" if head == "ori" else "location"))
        scores[head] = s
    return Conformal(alpha, "pmf" if "ori" in tabs else "error", "pmf" if "loc" in tabs else "error", scores["ori"], scores["loc"],
                     k_ori=k_ori, k_loc=k_loc, n_images=N, ori_beta=ps.ori_beta, loc_beta=ps.loc_beta)
