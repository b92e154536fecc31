"""Temperature scaling of the classification heads (Guo et al., 2017): calibrate() fits one scalar per head on held-out labelled data,
predict() / evaluate() / test_and_submit() apply it with calibration=....

Everything the project reports about a classification head -- ori_peak, ori_lambda, loc_peak, the ensemble's entropies, the fitted
modes -- is read off softmax(logits), and the soft-argmax orientation is a functional of that PMF too: a PMF that is too flat drags
q_est towards the mean of the bin grid.  The fit minimises the head's own training loss over beta = 1 / T; in beta the loss is convex:

    CE(beta) = sy lse(beta) - beta yz      dCE/dbeta = sy m1(beta) - yz      d2CE/dbeta2 = sy var(beta) >= 0
    sy = sum y    yz = sum y z    lse = log sum exp(beta z)    m1 = E_p[z]    var = Var_p[z]    p = softmax(beta z)

with z the fp32 logits of an image and y its fp32 encoded target (the PMF the loss uses; it may be un-normalised).  The fit is the
root of g(beta) = sum over the images of dCE/dbeta on [1/64, 64].  The logits never leave the device: urso_temp_stats evaluates a whole
dataset at up to 8 values of beta in one sweep, urso_temp_reduce adds the rows, and one [8, 4] table comes back per pass.

stats64 / reduce64 / scale32 are the three kernels in NumPy float64, the written specification (include/ursonet_train.h has the
reduction order of the device, which they do not reproduce: tests bound the difference by the operation count); fit64 is the search on
host arrays, fit_temperature the same search on device buffers.  Nothing here needs torch, the engine or the library before every
refusal of calibrate() has passed.
"""
import json
import math

import numpy as np

from .infer import Subset, refuse_launcher

MAX_J, COLS, TOTALS = 8, 26, 4                                   # URSO_TEMP_MAX_J, URSO_TEMP_COLS, URSO_TEMP_TOTALS (include/ursonet_train.h)
SY, YZ, LSE, M1, VAR = range(5)                                  # URSO_TEMP_* columns; LSE, M1, VAR of temperature j at + 3 j
BETA_MIN, BETA_MAX = 1.0 / 64, 64.0
GRID = tuple(2.0 ** k for k in range(-3, 5))                     # the first pass; GRID[3] is beta = 1
TOL = 1e-9                                                       # relative bracket width / Newton step at which the search stops
MAX_PASSES = 16
STATS_CHUNK = 4096                                               # rows per urso_temp_stats launch


# ------------------------------------------------------------------ the three kernels in NumPy float64
def stats64(z, y, betas):
    """urso_temp_stats on fp32 logits z [n, K] and fp32 targets y [n, K] at the inverse temperatures `betas` (1 .. 8): -> fp64
    [n, 2 + 3 J] = {SY, YZ, then LSE_j, M1_j, VAR_j}."""
    z, y = np.asarray(z, dtype=np.float32), np.asarray(y, dtype=np.float32)
    betas = [float(b) for b in betas]
    assert z.ndim == 2 and z.shape == y.shape and z.shape[1] >= 1 and 1 <= len(betas) <= MAX_J
    out = np.empty((z.shape[0], 2 + 3 * len(betas)))
    with np.errstate(all="ignore"):
        m = z.max(axis=1).astype(np.float64)                      # NaN-propagating
        z64, y64 = z.astype(np.float64), y.astype(np.float64)
        poison = 0.0 * m                                          # NaN unless m is finite
        out[:, SY] = y64.sum(axis=1) + poison
        out[:, YZ] = np.where(y == 0, 0.0, y64 * z64).sum(axis=1) + poison
        d = z64 - m[:, None]
        dd = d * d
        for j, b in enumerate(betas):
            e = np.exp(b * d)
            Z = e.sum(axis=1)
            A = np.where(e == 0, 0.0, e * d).sum(axis=1)          # a vanished term adds exactly 0, also for d = -inf
            Q = np.where(e == 0, 0.0, e * dd).sum(axis=1)
            r = A / Z
            out[:, LSE + 3 * j] = np.log(Z) + b * m
            out[:, M1 + 3 * j] = m + r
            out[:, VAR + 3 * j] = Q / Z - r * r
    return out


def row_terms(rows, betas):
    """(CE, g, h) [n, J] each, the per-row terms of urso_temp_reduce in its operation order, and bad [n, J]: a statistic is not finite."""
    rows = np.asarray(rows, dtype=np.float64)
    b = np.asarray([float(x) for x in betas])
    J = len(b)
    sy, yz = rows[:, SY:SY + 1], rows[:, YZ:YZ + 1]
    lse, m1, var = (rows[:, c:c + 3 * J:3] for c in (LSE, M1, VAR))
    with np.errstate(all="ignore"):
        ce, g, h = sy * lse - b[None, :] * yz, sy * m1 - yz, sy * var
    bad = ~(np.isfinite(sy) & np.isfinite(yz) & np.isfinite(lse) & np.isfinite(m1) & np.isfinite(var))
    return ce, g, h, bad


def reduce64(rows, betas):
    """urso_temp_reduce: -> [J, 4] = {sum CE, sum g, sum h, rows that are not finite} over all rows of a stats64 table."""
    ce, g, h, bad = row_terms(rows, betas)
    with np.errstate(all="ignore"):
        return np.stack([ce.sum(axis=0), g.sum(axis=0), h.sum(axis=0), bad.sum(axis=0).astype(np.float64)], axis=1)


def scale32(z, beta):
    """urso_temp_scale: fl32(z * beta), the product taken in fp64 (exact there), rounded once."""
    with np.errstate(all="ignore"):
        return (np.asarray(z, dtype=np.float32).astype(np.float64) * float(beta)).astype(np.float32)


# ------------------------------------------------------------------ the search
def _between(lo, hi, k, parts):
    """The k-th of the points that cut [lo, hi] into `parts` equal pieces in log beta."""
    return lo * (hi / lo) ** (k / float(parts))


def search(evaluate, n_rows, max_passes=MAX_PASSES, tol=TOL):
    """The root of g on [BETA_MIN, BETA_MAX].  evaluate(betas) -> [J, 4] totals (reduce64's) for 1 .. 8 values of beta: one sweep over
    the data, a pass.  -> (beta, info).

    Pass 1 is GRID.  g does not decrease in beta (the loss is convex), so the signs give a bracket [lo, hi] of ratio 2 -- or, where the
    grid does not hold the root, the piece between the grid and the bound, whose g is not known yet.  Every later pass evaluates 7 points
    that cut the bracket into 8 equal pieces in log beta and, as the eighth, the bound whose g is unknown or else the Newton point
    beta - g / h from the bracket end with the smaller |g| (a point that falls outside the bracket is replaced by the middle of the piece
    next to that end).  The bracket shrinks at least 8-fold per pass whatever Newton does: from log 8 to below 1e-9 in 11 passes; the last
    pass evaluates the loss at the answer.  It stops when the bracket is at most tol wide, relative, or the Newton step is at most tol of
    beta; the answer is then the Newton point (inside the bracket) or the bracket's geometric middle."""
    assert max_passes >= 3
    info = dict(passes=0, clamped=False, flat=False, converged=False, n_rows=int(n_rows))
    seen = {}

    def run(betas):
        t = np.asarray(evaluate(betas), dtype=np.float64).reshape(len(betas), TOTALS)
        info["passes"] += 1
        if not np.all(np.isfinite(t)) or np.any(t[:, 3] != 0):
            raise ValueError("calibration: %d of %d rows are not finite (a NaN or infinite logit, or a target that weighs a -inf bin); "
                             "the totals at beta = %s are %s" % (int(np.nanmax(t[:, 3])), n_rows, list(betas), t[:, :3].tolist()))
        for b, row in zip(betas, t):
            seen[float(b)] = (float(row[0]), float(row[1]), float(row[2]))
        return t

    def done(beta, **kw):
        info.update(kw)
        if beta not in seen:
            run([beta])
        ce, g, h = seen[beta]
        info.update(beta=beta, nll_before=seen[1.0][0] / max(n_rows, 1), nll_after=ce / max(n_rows, 1), g=g, h=h)
        return beta, info

    t = run(GRID)
    if np.all(t[:, 2] == 0):                                      # every row's logits are equal: the loss does not depend on beta
        return done(1.0, flat=True, converged=True)
    lo, hi = BETA_MIN, BETA_MAX                                   # ends not in `seen`: g unknown
    while info["passes"] < max_passes - 1:
        for b, (_ce, g, _h) in seen.items():
            if g == 0:
                return done(b, converged=True)
            if g < 0 and b > lo:
                lo = b
            if g > 0 and b < hi:
                hi = b
        if BETA_MIN in seen and seen[BETA_MIN][1] > 0:            # the loss still rises at the lower bound
            return done(BETA_MIN, clamped=True, converged=True)
        if BETA_MAX in seen and seen[BETA_MAX][1] < 0:
            return done(BETA_MAX, clamped=True, converged=True)
        newton, best = None, None
        if lo in seen and hi in seen:
            best = lo if abs(seen[lo][1]) <= abs(seen[hi][1]) else hi
            _ce, g, h = seen[best]
            if h > 0 and math.isfinite(g / h) and lo <= best - g / h <= hi:     # (a step below an ulp of beta leaves the end where it is)
                newton = best - g / h
            if newton is not None and abs(newton - best) <= tol * best:
                return done(newton, converged=True, bracket=(lo, hi))
            if hi - lo <= tol * lo:
                return done(newton if newton is not None else math.sqrt(lo * hi), converged=True, bracket=(lo, hi))
            if newton is None:
                newton = _between(lo, hi, 0.5, 8) if best == lo else _between(lo, hi, 7.5, 8)
        extra = lo if lo not in seen else (hi if hi not in seen else newton)
        run(sorted(set([extra] + [_between(lo, hi, k, 8) for k in range(1, 8)])))
    return done(math.sqrt(lo * hi), bracket=(lo, hi))


def fit64(z, y, max_passes=MAX_PASSES, tol=TOL):
    """The search on host arrays: fp32 logits z [N, K] and fp32 encoded targets y [N, K] -> (beta, info).  info: passes, clamped (the
    root lies outside [1/64, 64] and beta is the bound), flat (every row's logits are equal: beta = 1), converged, nll_before / nll_after
    (the mean CE per row at beta = 1 and at the fit), g and h at the fit.  ValueError: a total that is not finite, with the number of rows."""
    z, y = np.asarray(z, dtype=np.float32), np.asarray(y, dtype=np.float32)
    return search(lambda betas: reduce64(stats64(z, y, betas), betas), z.shape[0], max_passes, tol)


def fit_temperature(z_dev, y_dev, max_passes=MAX_PASSES, tol=TOL):
    """The search of fit64 on fp32 device tensors [N, K] with contiguous rows: urso_temp_stats per chunk of rows, urso_temp_reduce per
    pass, and one [8, 4] table read back per pass -> (beta, info)."""
    import torch
    from . import hip
    N = int(z_dev.shape[0])
    assert N >= 1 and tuple(z_dev.shape) == tuple(y_dev.shape)
    rows = torch.empty(N, hip.TEMP_COLS, dtype=torch.float64, device=z_dev.device)
    totals = torch.empty(hip.TEMP_MAX_J, hip.TEMP_TOTALS, dtype=torch.float64, device=z_dev.device)

    def evaluate(betas):
        for r0 in range(0, N, STATS_CHUNK):
            n = min(STATS_CHUNK, N - r0)
            hip.temp_stats(n, n, r0, betas, z_dev[r0:r0 + n], y_dev[r0:r0 + n], rows)
        hip.temp_reduce(N, betas, rows, totals)
        return totals.cpu().numpy()[:len(betas)]
    return search(evaluate, N, max_passes, tol)


# ------------------------------------------------------------------ the result
def _beta(name, v):
    if v is None:
        return None
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(v, bool) or not (0 < f < float("inf")):
        raise ValueError("Calibration: %s must be a finite number > 0 or None (got %r)" % (name, v))
    return f


class Calibration(object):
    """The fitted inverse temperatures of a model's classification heads: ori_beta / loc_beta (None: the head is a regression head, or
    is left as it is), ori_temperature / loc_temperature (1 / beta), k_ori / k_loc (the heads' bin counts; None on a calibration built by
    hand, which then fits any model), n_images, and per head the fit's report ori_fit / loc_fit: a dict of nll_before, nll_after (mean
    CE per image at beta = 1 and at the fit), passes, clamped, flat, converged -- also as ori_nll_before, loc_passes, ... (None without a
    fit).  save(path) / Calibration.load(path): JSON, floats by repr, so they come back bit for bit."""
    FIT_KEYS = ("nll_before", "nll_after", "passes", "clamped", "flat", "converged")

    def __init__(self, ori_beta=None, loc_beta=None, k_ori=None, k_loc=None, n_images=None, ori_fit=None, loc_fit=None):
        self.ori_beta, self.loc_beta = _beta("ori_beta", ori_beta), _beta("loc_beta", loc_beta)
        self.k_ori, self.k_loc = (None if k is None else int(k) for k in (k_ori, k_loc))
        self.n_images = None if n_images is None else int(n_images)
        self.ori_fit = None if ori_fit is None else dict((k, ori_fit[k]) for k in self.FIT_KEYS)
        self.loc_fit = None if loc_fit is None else dict((k, loc_fit[k]) for k in self.FIT_KEYS)

    ori_temperature = property(lambda self: None if self.ori_beta is None else 1.0 / self.ori_beta)
    loc_temperature = property(lambda self: None if self.loc_beta is None else 1.0 / self.loc_beta)

    def __getattr__(self, name):                                  # ori_nll_before, loc_passes, ...
        head, _, key = name.partition("_")
        if head in ("ori", "loc") and key in self.FIT_KEYS:
            fit = self.__dict__.get(head + "_fit")
            return None if fit is None else fit[key]
        raise AttributeError(name)

    def to_dict(self):
        return dict(ori_beta=self.ori_beta, loc_beta=self.loc_beta, k_ori=self.k_ori, k_loc=self.k_loc, n_images=self.n_images,
                    ori_fit=self.ori_fit, loc_fit=self.loc_fit)

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
        return isinstance(other, Calibration) and self.to_dict() == other.to_dict()

    def __repr__(self):
        return "Calibration(%s)" % ", ".join("%s=%r" % kv for kv in sorted(self.to_dict().items()) if kv[1] is not None)

    def line(self):
        """The line evaluate(calibration=...) prints behind its usual ones."""
        parts = ["%s T = %s (beta %s)" % (name, 1.0 / b, b) for name, b in (("orientation", self.ori_beta), ("location", self.loc_beta))
                 if b is not None]
        return "Calibration: " + (", ".join(parts) if parts else "no head is scaled")

    def check_model(self, k_ori, k_loc, who="predict"):
        """ValueError where this calibration does not fit a model whose classification heads have k_ori / k_loc bins (0: a regression head)."""
        for name, beta, mine, model in (("ori", self.ori_beta, self.k_ori, k_ori), ("loc", self.loc_beta, self.k_loc, k_loc)):
            if beta is not None and not model:
                raise ValueError("%s: the calibration has %s_beta = %r, but the model's %s head is a regression head: there are no logits "
                                 "to scale" % (who, name, beta, "orientation" if name == "ori" else "location"))
            if beta is not None and mine is not None and mine != model:
                raise ValueError("%s: the calibration was fitted on a %s head of %d bins, the model's has %d" % (who, name, mine, model))


def check_calibration(calibration, members=None, who="predict"):
    """The refusals of predict / evaluate / test_and_submit (calibration=...) that need neither the model nor a GPU."""
    if calibration is None:
        return None
    if not isinstance(calibration, Calibration):
        raise ValueError("%s: calibration must be a calibrate.Calibration (from calibrate(), Calibration.load() or Calibration(ori_beta=..., "
                         "loc_beta=...)), got %s" % (who, type(calibration).__name__))
    if members is not None:
        raise ValueError("%s: calibration=... cannot be combined with members=...: a temperature belongs to one weight set; calibrate and "
                         "predict each member on its own" % who)
    return calibration


# ------------------------------------------------------------------ the fit over a dataset
def buffer_bytes(N, k_ori, k_loc):
    """Device bytes of the whole-dataset buffers of calibrate(): per classification head the fp32 logits and the fp32 encoded targets,
    N * K * 8 bytes."""
    return N * (k_ori + k_loc) * 8


def check_size(N, k_ori, k_loc, max_gb, who="calibrate"):
    """ValueError, naming the figure, when the fit would hold more than max_gb GiB on the device."""
    try:
        limit = float(max_gb)
    except (TypeError, ValueError):
        limit = float("nan")
    if not limit > 0:
        raise ValueError("%s: max_gb must be a number > 0 (got %r)" % (who, max_gb))
    need = buffer_bytes(N, k_ori, k_loc)
    if need > limit * 2 ** 30:
        raise ValueError("%s: the logits and targets of %d images (%d orientation and %d location bins in fp32) need %.3f GiB on the "
                         "device, more than max_gb = %g; calibrate on fewer images (nr_images) or raise max_gb"
                         % (who, N, k_ori, k_loc, need / 2.0 ** 30, limit))
    return need


def calibrate(model, dataset, nr_images=None, workers=None, cache=None, max_gb=16, *, members=None, views=None):
    """Fits the temperature of every classification head of an inference model on a labelled dataset -> Calibration.  The dataset is
    walked once (the first nr_images of dataset.image_ids; None: all) with evaluate()'s feeder and inference pass; each head's fp32
    logits and stored encoded targets are kept in whole-dataset device buffers (N * K * 8 bytes per head, at most max_gb GiB), then each
    head is fitted by fit_temperature.  The model's weights and state are not touched.  ValueError, before any GPU work: a model without
    a classification head, a data-parallel launcher, members or views (calibrate the one model that will predict), no labelled image,
    buffers above max_gb (the message names their size); during the fit: rows that are not finite."""
    who = "calibrate"
    if members is not None or views is not None:
        raise ValueError("%s: members=... and views=... are not supported: a temperature belongs to one weight set and the plain pass; "
                         "calibrate and predict each member on its own" % who)
    refuse_launcher(model, who, "fit the whole dataset")
    assert model.mode == "inference", "Create model in inference mode."
    cfg = model.config
    soft, loc_class = not (cfg.REGRESS_ORI or cfg.REGRESS_KEYPOINTS), not cfg.REGRESS_LOC
    if not (soft or loc_class):
        raise ValueError("%s: the model has no classification head (REGRESS_ORI and REGRESS_LOC are both set): there is no PMF to "
                         "calibrate" % who)
    from .infer import check_heads
    check_heads(model, dataset, False, who)
    ids = list(dataset.image_ids)
    if nr_images is not None:
        if int(nr_images) < 1:
            raise ValueError("%s: nr_images must be >= 1 or None (got %r)" % (who, nr_images))
        ids = ids[:int(nr_images)]
    N = len(ids)
    if N < 1:
        raise ValueError("%s: the dataset has no images" % who)
    from .ensemble import head_bins
    k_ori, k_loc = head_bins(model)
    check_size(N, k_ori, k_loc, max_gb, who)                       # before any GPU work

    from .feeder import EvalFeeder
    from .infer import PosePass, loader_workers
    ps = PosePass(model, dataset, False, who=who)
    torch, dev = ps.torch, ps.dev
    f32 = dict(dtype=torch.float32, device=dev)
    z_ori, y_ori = (torch.empty(N, k_ori, **f32), torch.empty(N, k_ori, **f32)) if soft else (None, None)
    z_loc, y_loc = (torch.empty(N, k_loc, **f32), torch.empty(N, k_loc, **f32)) if loc_class else (None, None)
    feed = EvalFeeder(model, Subset(dataset, ids) if nr_images is not None else dataset, ps.cfg, enc_loc=loc_class, enc_ori=soft,
                      workers=loader_workers(ps.cfg, workers), cache=cache)
    try:
        for bt in feed:
            ps.run(bt.images)
            loc, rest = ps.eng.outputs()
            sl = slice(bt.row0, bt.row0 + bt.n)
            if soft:                                               # the staging buffers are the feeder's, the outputs the engine's: both move
                z_ori[sl].copy_(rest[:bt.n]); y_ori[sl].copy_(bt.enc_ori[:bt.n])
            if loc_class:
                z_loc[sl].copy_(loc[:bt.n]); y_loc[sl].copy_(bt.enc_loc[:bt.n])
    finally:
        feed.close()
    fits = {}
    for name, z, y in (("ori", z_ori, y_ori), ("loc", z_loc, y_loc)):
        if z is not None:
            try:
                fits[name] = fit_temperature(z, y)
            except ValueError as e:
                raise ValueError("%s: the %s head: %s" % (who, "orientation" if name == "ori" else "location", e))
    ori, loc = fits.get("ori"), fits.get("loc")
    return Calibration(ori_beta=ori[0] if ori else None, loc_beta=loc[0] if loc else None, k_ori=k_ori or None, k_loc=k_loc or None,
                       n_images=N, ori_fit=ori[1] if ori else None, loc_fit=loc[1] if loc else None)
