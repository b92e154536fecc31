"""Feature-space domain-shift scores (Lee et al., 2018: Mahalanobis distance in feature space; Frechet distance between two domains):
fit_domain() turns unlabelled images of the source domain into the mean, covariance and whitening matrix of their pooled bottleneck
features, predict() / evaluate() with domain=... give every image its squared Mahalanobis distance to that domain (and, with a held-out
source set, the conformal p-value of "this frame is exchangeable with the source"), domain_gap() gives the Frechet distance between two
fitted domains -- the label-free number for the gap between rendered and real frames.

The feature row of an image is the mean of the bottleneck_layer output (Engine.features(): [h, w, C], the tensor both head trunks read)
over the cells of a grid (gh, gw) that divides (h, w): D = gh * gw * C values, feature ((gy * gw) + gx) * C + c.

pool64 / gram_add64 / maha64 are the three kernels (urso_feat_pool / urso_feat_gram_add / urso_feat_maha, include/ursonet_feat.h) in NumPy
float64, and settle() is the host's part: together the written specification.  No transcendental function is involved and every sum has
one stated order, so the kernels equal the statements bit for bit.  The statistics are a function of the image order alone, whatever the
batch size: the centre is a bit copy of the first image's feature row, and rows are added one behind the other.  Nothing here needs
torch, the engine or the library before every refusal has passed.
"""

import numpy as np

from .infer import Subset, refuse_launcher

MAX_D, COLS, MAHA_ROWS = 4096, 4, 8                               # URSO_FEAT_MAX_D, URSO_FEAT_COLS, URSO_FEAT_MAHA_ROWS (include/ursonet_feat.h)
SCORE, DIST2, ZMAX, ZARG = range(4)                               # the score row


# ------------------------------------------------------------------ the three kernels in NumPy
def check_grid(geometry, grid, who="fit_domain"):
    """(gh, gw, D) of a grid over the feature geometry (h, w, C); ValueError where it does not divide (h, w) or D exceeds MAX_D."""
    h, w, C = (int(v) for v in geometry)
    try:
        gh, gw = (int(v) for v in grid)
    except (TypeError, ValueError):
        raise ValueError("%s: grid must be a pair (gh, gw) (got %r)" % (who, grid))
    if gh < 1 or gw < 1 or h % gh or w % gw:
        raise ValueError("%s: the grid %r does not divide the model's feature map of %d x %d cells" % (who, (gh, gw), h, w))
    D = gh * gw * C
    if D > MAX_D:
        raise ValueError("%s: the grid %r over %d channels gives D = %d features, more than URSO_FEAT_MAX_D = %d; use a coarser grid"
                         % (who, (gh, gw), C, D, MAX_D))
    return gh, gw, D


def pool64(act, grid):
    """urso_feat_pool: act [n, h, w, C] (any float dtype NumPy has; the conversion to fp64 is exact) -> fp64 [n, gh * gw * C]: per cell and
    channel the sum over the cell's pixels in row-major ascending order from +0.0, then one division by the pixel count."""
    a = np.asarray(act).astype(np.float64)
    n, h, w, C = a.shape
    gh, gw, D = check_grid((h, w, C), grid, "pool64")
    ch, cw = h // gh, w // gw
    cells = a.reshape(n, gh, ch, gw, cw, C)
    s = np.zeros((n, gh, gw, C))
    with np.errstate(all="ignore"):
        for y in range(ch):
            for x in range(cw):
                s = s + cells[:, :, y, :, x, :]
        return (s / float(ch * cw)).reshape(n, D)


def gram_add64(X, centre, s, G):
    """urso_feat_gram_add, in place: for the rows of X [n, D] ascending, d = X[r] - centre; s += d; G += triu(outer(d, d)) -- the upper
    triangle including the diagonal (what the statement adds below it is +0.0: the kernel neither reads nor writes there)."""
    X, c = np.asarray(X, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    assert X.ndim == 2 and c.shape == (X.shape[1],) == s.shape and G.shape == (X.shape[1],) * 2 and s.dtype == G.dtype == np.float64
    with np.errstate(all="ignore"):
        for r in range(X.shape[0]):
            d = X[r] - c
            s += d
            G += np.triu(np.outer(d, d))
    return s, G


def maha64(X, mean, W):
    """urso_feat_maha: X [n, D] against mean [D] and the lower-triangular W [D, D] (nothing above the diagonal is read) -> fp64 [n, 4] =
    {SCORE, DIST2, ZMAX, ZARG}: d = X - mean; y_i = sum_{j <= i} W_ij d_j, j ascending from +0.0, acc = acc + W_ij * d_j; SCORE = sum y_i^2,
    DIST2 = sum d_i^2, both i ascending; ZMAX = max |y_i| at its lowest index ZARG.  A row of X that is not finite is NaN throughout."""
    X, mean, W = (np.asarray(v, dtype=np.float64) for v in (X, mean, W))
    n, D = X.shape
    assert mean.shape == (D,) and W.shape == (D, D)
    out = np.zeros((n, COLS))
    y, zmax = np.zeros((n, D)), np.full(n, -1.0)
    with np.errstate(all="ignore"):
        d = X - mean
        for j in range(D):
            y[:, j:] = y[:, j:] + W[j:, j][None, :] * d[:, j][:, None]     # y_j is complete behind this step
            out[:, SCORE] = out[:, SCORE] + y[:, j] * y[:, j]
            out[:, DIST2] = out[:, DIST2] + d[:, j] * d[:, j]
            a = np.abs(y[:, j])
            up = (a > zmax) | (np.isnan(a) & ~np.isnan(zmax))
            zmax = np.where(up, a, zmax)
            out[:, ZARG] = np.where(up, float(j), out[:, ZARG])
    out[:, ZMAX] = zmax
    out[~np.all(np.isfinite(X), axis=1)] = np.nan
    return out


# ------------------------------------------------------------------ the host's part
def oas_rho(S, n):
    """The oracle-approximating shrinkage weight of Chen et al. (2010) for a sample covariance S [D, D] of n rows:
    min(1, ((1 - 2/D) tr(S^2) + tr(S)^2) / ((n + 1 - 2/D) (tr(S^2) - tr(S)^2 / D))), and 1 where the denominator is <= 0."""
    S = np.asarray(S, dtype=np.float64)
    D = S.shape[0]
    tr, tr2 = float(np.trace(S)), float(np.sum(S * S))
    den = (n + 1.0 - 2.0 / D) * (tr2 - tr * tr / D)
    if not den > 0:
        return 1.0
    return float(min(1.0, ((1.0 - 2.0 / D) * tr2 + tr * tr) / den))


def _shrink(shrink, who="fit_domain"):
    if isinstance(shrink, str):
        if shrink != "oas":
            raise ValueError("%s: shrink is 'oas' or a number in [0, 1] (got %r)" % (who, shrink))
        return shrink
    try:
        f = float(shrink)
    except (TypeError, ValueError):
        f = float("nan")
    if isinstance(shrink, bool) or not (0 <= f <= 1):
        raise ValueError("%s: shrink is 'oas' or a number in [0, 1] (got %r)" % (who, shrink))
    return f


def settle(centre, s, G, n, shrink="oas", who="fit_domain"):
    """The accumulators of n rows -> (mean, cov, rho, W), in float64: mean = centre + s / n; cov_ij = (G_ij - s_i s_j / n) / (n - 1) from the
    upper triangle, mirrored; S' = (1 - rho) cov + rho (tr cov / D) I with rho = oas_rho or the given number; L = cholesky(S');
    W = tril(solve(L, I)), so that W S' W^T = I.  ValueError: n < 2, or an S' that is not positive definite."""
    shrink = _shrink(shrink, who)
    centre, s, G = (np.asarray(v, dtype=np.float64) for v in (centre, s, G))
    D = centre.shape[0]
    if n < 2:
        raise ValueError("%s: a covariance needs at least 2 images (got %d): raise nr_images or pass a larger dataset" % (who, n))
    mean = centre + s / n
    up = np.triu((G - np.outer(s, s) / n) / (n - 1.0))
    cov = up + np.triu(up, 1).T
    rho = oas_rho(cov, n) if shrink == "oas" else shrink
    Sp = (1.0 - rho) * cov + rho * (np.trace(cov) / D) * np.eye(D)
    try:
        L = np.linalg.cholesky(Sp)
    except np.linalg.LinAlgError:
        raise ValueError("%s: the shrunk covariance of %d images in %d dimensions (shrink %r) is not positive definite: raise shrink "
                         "(or use 'oas'), raise nr_images above D, or use a coarser grid" % (who, n, D, rho))
    W = np.tril(np.linalg.solve(L, np.eye(D)))
    return mean, cov, float(rho), W


def spearman(a, b):
    """Spearman's rho of two vectors: Pearson's correlation of their average ranks (NaN where a rank vector is constant)."""
    def rank(v):
        _u, inv, cnt = np.unique(np.asarray(v, dtype=np.float64), return_inverse=True, return_counts=True)
        return (np.cumsum(cnt) - (cnt - 1) / 2.0)[inv.reshape(-1)]
    ra, rb = rank(a), rank(b)
    ra, rb = ra - ra.mean(), rb - rb.mean()
    den = np.sqrt(np.sum(ra * ra) * np.sum(rb * rb))
    return float(np.sum(ra * rb) / den) if den > 0 else float("nan")


# ------------------------------------------------------------------ the result
def feature_geometry(config):
    """(h, w, C) of the bottleneck features of a model with this config (Graph.feat), without torch or the engine."""
    from .graph import build_graph
    f = build_graph(config).feat
    return int(f.h), int(f.w), int(f.c)


class Domain(object):
    """The feature statistics of a source domain: n images, D = gh * gw * C features over `grid` = (gh, gw) of the feature geometry
    `geometry` = (h, w, C); centre (the first image's feature row), mean [D], cov [D, D] (the sample covariance), shrink (the gamma used),
    W [D, D] lower triangular with W S' W^T = I for the shrunk covariance S', and holdout_scores: the sorted scores of held-out source
    images (None: no holdout, no p-values).  save(path) / Domain.load(path): .npz, bit for bit."""
    ARRAYS = ("centre", "mean", "cov", "W")

    def __init__(self, n, grid, geometry, centre, mean, cov, shrink, W, holdout_scores=None):
        self.n, self.grid, self.geometry = int(n), tuple(int(v) for v in grid), tuple(int(v) for v in geometry)
        self.D = check_grid(self.geometry, self.grid, "Domain")[2]
        self.shrink = float(shrink)
        for name, v, shape in (("centre", centre, (self.D,)), ("mean", mean, (self.D,)), ("cov", cov, (self.D, self.D)), ("W", W, (self.D, self.D))):
            v = np.array(v, dtype=np.float64)
            if v.shape != shape:
                raise ValueError("Domain: %s has shape %r, D = %d needs %r" % (name, v.shape, self.D, shape))
            setattr(self, name, v)
        self.holdout_scores = None if holdout_scores is None else np.sort(np.asarray(holdout_scores, dtype=np.float64).reshape(-1))

    def p_value(self, scores):
        """(1 + #{holdout >= score}) / (m + 1): the conformal p-value of "this frame is exchangeable with the source" (NaN for a NaN score)."""
        if self.holdout_scores is None:
            raise ValueError("Domain.p_value needs holdout scores: fit_domain(..., holdout=a second dataset of the source domain)")
        s = np.asarray(scores, dtype=np.float64)
        m = len(self.holdout_scores)
        p = (1.0 + (m - np.searchsorted(self.holdout_scores, s, side="left"))) / (m + 1.0)
        return np.where(np.isnan(s), np.nan, p)

    def save(self, path):
        d = dict((k, getattr(self, k)) for k in self.ARRAYS)
        d.update(n=np.int64(self.n), grid=np.array(self.grid, dtype=np.int64), geometry=np.array(self.geometry, dtype=np.int64),
                 shrink=np.float64(self.shrink))
        if self.holdout_scores is not None:
            d["holdout_scores"] = self.holdout_scores
        with open(path, "wb") as f:
            np.savez(f, **d)
        return path

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            return cls(int(z["n"]), z["grid"], z["geometry"], z["centre"], z["mean"], z["cov"], float(z["shrink"]), z["W"],
                       z["holdout_scores"] if "holdout_scores" in z.files else None)

    def __eq__(self, other):
        if not isinstance(other, Domain) or (self.n, self.grid, self.geometry) != (other.n, other.grid, other.geometry):
            return False
        bits = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)      # noqa: E731
        pairs = [(getattr(self, k), getattr(other, k)) for k in self.ARRAYS + ("holdout_scores",)] + [(np.float64(self.shrink), np.float64(other.shrink))]
        return all((a is None) == (b is None) and (a is None or np.array_equal(bits(a), bits(b))) for a, b in pairs)

    __hash__ = None

    def __repr__(self):
        return "Domain(n=%d, D=%d, grid=%r, geometry=%r, shrink=%r, holdout=%s)" % (
            self.n, self.D, self.grid, self.geometry, self.shrink, "None" if self.holdout_scores is None else "<%d>" % len(self.holdout_scores))

    def check_model(self, model, who="predict"):
        """ValueError where the model's feature geometry is not the one the domain was fitted on."""
        geo = feature_geometry(model.config)
        if geo != self.geometry:
            raise ValueError("%s: the domain was fitted on bottleneck features of %d x %d cells with %d channels, this model's have %d x %d "
                             "cells with %d channels: run fit_domain() on this model" % ((who,) + self.geometry + geo))

    def line(self, res):
        """The line evaluate(domain=...) prints behind its usual ones: the median and 95th percentile of the score, with a holdout the share
        of images with p < 0.05, and Spearman's rho of the score with the two errors (does the score predict the error?)."""
        s = np.asarray(res.domain_score, dtype=np.float64)
        txt = "Domain: score median %s, 95th percentile %s" % ((np.median(s), np.percentile(s, 95)) if len(s) else (float("nan"),) * 2)
        if res.domain_p is not None:
            txt += ", p < 0.05 for %s of the images" % (np.mean(res.domain_p < 0.05) if len(s) else float("nan"))
        return txt + "; Spearman's rho of the score with ori_err %s, with loc_err %s (D = %d, %d source images)" % (
            spearman(s, res.ori_err), spearman(s, res.loc_err), self.D, self.n)


def check_domain(domain, members=None, views=None, who="predict"):
    """The refusals of predict / evaluate (domain=...) that need neither the model nor a GPU."""
    if domain is None:
        return None
    if not isinstance(domain, Domain):
        raise ValueError("%s: domain must be a domain.Domain (from fit_domain() or Domain.load()), got %s" % (who, type(domain).__name__))
    if members is not None or views is not None:
        raise ValueError("%s: domain=... cannot be combined with members=... or views=...: the statistics were fitted on the plain pass of "
                         "one weight set" % who)
    refuse_launcher(None, "%s: domain=..." % who, "walk the whole dataset")
    return domain


def domain_fields(res, dom, table):
    """Sets domain_score, domain_dist2, domain_zmax, domain_zarg and domain_p (None without a holdout) on a result from the pass's rows."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, COLS)
    res.domain_score, res.domain_dist2, res.domain_zmax = t[:, SCORE].copy(), t[:, DIST2].copy(), t[:, ZMAX].copy()
    res.domain_zarg = np.where(np.isnan(t[:, ZARG]), -1, t[:, ZARG]).astype(np.int32)
    res.domain_p = None if dom.holdout_scores is None else dom.p_value(res.domain_score)


def no_domain_fields(res):
    res.domain_score = res.domain_dist2 = res.domain_zmax = res.domain_zarg = res.domain_p = None


def domain_gap(a, b):
    """The Frechet distance between two fitted domains of equal geometry and grid, in host float64:
    |mu_a - mu_b|^2 + tr(Sa + Sb - 2 (Sa Sb)^(1/2)) -> {"frechet", "mean_term", "cov_term"}.  The trace of the root is the sum of the
    square roots of the eigenvalues (eigh, negative ones clamped to 0) of Sa^(1/2) Sb Sa^(1/2), Sa^(1/2) from eigh of Sa."""
    for v in (a, b):
        if not isinstance(v, Domain):
            raise ValueError("domain_gap: needs two domain.Domain (got %s)" % type(v).__name__)
    if (a.geometry, a.grid) != (b.geometry, b.grid):
        raise ValueError("domain_gap: the two domains differ in geometry or grid: %r %r against %r %r" % (a.geometry, a.grid, b.geometry, b.grid))
    dm = a.mean - b.mean
    w, V = np.linalg.eigh(a.cov)
    R = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = R @ b.cov @ R
    ev = np.linalg.eigvalsh((M + M.T) / 2.0)
    mean_term = float(np.sum(dm * dm))
    cov_term = float(np.trace(a.cov) + np.trace(b.cov) - 2.0 * np.sum(np.sqrt(np.maximum(ev, 0.0))))
    return {"frechet": mean_term + cov_term, "mean_term": mean_term, "cov_term": cov_term}


# ------------------------------------------------------------------ on the device
class DomainPass(object):
    """The launches of one command on a PosePass ps for a fitted Domain: the batch's feature rows (fp64 [B, D], urso_feat_pool) and a fp64
    device table [rows, 4] of scores (urso_feat_maha).  Nothing here synchronises; table() reads once, at the end."""

    def __init__(self, ps, rows, dom):
        hip, torch = ps.hip, ps.torch
        hip.side_lib("feat")                                       # a missing library is an error here, not in the first batch
        self.ps, self.hip, self.grid = ps, hip, dom.grid
        self.x = ps.table(ps.B, dom.D)
        self.out = ps.table(rows, hip.FEAT_COLS)
        self.mean = torch.as_tensor(dom.mean).to(ps.dev).contiguous()
        self.wt = hip.feat_whiten_t(dom.W, ps.dev)

    def launch(self, n, row0):
        """Behind run(): the n valid images' rows [row0, row0 + n) of the score table."""
        ps, hip = self.ps, self.hip
        hip.feat_pool(ps.B, n, 0, self.grid, ps.eng.features(), self.x)
        hip.feat_maha(ps.B, n, row0, self.x, self.mean, self.wt, self.out)

    def table(self, N):
        return self.out[:N].cpu().numpy()


def _plan(model, dataset, nr_images, grid, shrink, max_gb, who):
    """Every refusal of fit_domain() that needs no GPU -> (ids, geometry, grid, D)."""
    _shrink(shrink, who)
    refuse_launcher(model, who, "walk the whole dataset")
    if model.mode != "inference":
        raise ValueError("%s needs a model created in inference mode (got mode %r): the features are those predict() computes" % (who, model.mode))
    geo = feature_geometry(model.config)
    gh, gw, D = check_grid(geo, grid, who)
    ids = list(dataset.image_ids)
    if nr_images is not None:
        if int(nr_images) < 2:
            raise ValueError("%s: nr_images must be >= 2 or None (got %r): a covariance needs two images" % (who, nr_images))
        ids = ids[:int(nr_images)]
    B = int(model.config.BATCH_SIZE)
    need = 8 * (D * D + 3 * D + B * D) + 8 * COLS * len(ids)
    if need > float(max_gb) * 2 ** 30:
        raise ValueError("%s: the accumulators for D = %d features need %d bytes (%.3g GiB), more than max_gb = %r GiB; use a coarser grid or "
                         "raise max_gb" % (who, D, need, need / 2.0 ** 30, max_gb))
    if len(ids) < 2:
        raise ValueError("%s: a covariance needs at least 2 images (the dataset has %d): pass a larger dataset" % (who, len(ids)))
    return ids, geo, (gh, gw), D


def fit_domain(model, dataset, holdout=None, nr_images=None, grid=(1, 1), shrink="oas", workers=None, cache=None, max_gb=16):
    """The feature statistics of the source domain -> Domain.  model: an inference model; dataset: unlabelled images (only load_image is
    called), walked once (the first nr_images of dataset.image_ids; None: all) with predict()'s feeder and inference pass: behind each
    batch's forward pass urso_feat_pool writes the valid images' feature rows, the first image's row becomes the centre (a bit copy), and
    urso_feat_gram_add adds the rows into s and the upper triangle of G on the device; the accumulators are read back once, and settle()
    gives the mean, the covariance and the whitening matrix W of the shrunk covariance (shrink: "oas", or a number in [0, 1]).  holdout: a
    second dataset of the SOURCE domain, not used for the fit: a second walk scores it (urso_feat_maha) and its sorted scores are kept
    for Domain.p_value.  ValueError, before any GPU work: a grid that does not divide the model's feature map, D > 4096, accumulators above
    max_gb GiB, a training-mode model, a data-parallel launcher, fewer than 2 images; behind the walk: features that are not finite (the
    message names the first offending image rows), a shrunk covariance that is not positive definite."""
    who = "fit_domain"
    ids, geo, grid, D = _plan(model, dataset, nr_images, grid, shrink, max_gb, who)
    N = len(ids)
    from .feeder import EvalFeeder
    from .infer import PosePass, loader_workers
    ps = PosePass(model, dataset, False, who=who)
    hip, torch = ps.hip, ps.torch
    hip.side_lib("feat")
    f64 = dict(dtype=torch.float64, device=ps.dev)
    x, centre, s, G = ps.table(ps.B, D), torch.zeros(D, **f64), torch.zeros(D, **f64), torch.zeros(D, D, **f64)
    plan = []
    finite = torch.ones((N + ps.B - 1) // ps.B, dtype=torch.bool, device=ps.dev)
    feed = EvalFeeder(model, Subset(dataset, ids) if nr_images is not None else dataset, ps.cfg, workers=loader_workers(ps.cfg, workers),
                      labels=False, cache=cache)
    try:
        for bt in feed:
            ps.run(bt.images)
            hip.feat_pool(ps.B, bt.n, 0, grid, ps.eng.features(), x)
            if bt.row0 == 0:
                centre.copy_(x[0])                                 # the bits of the first image's row
            hip.feat_gram_add(ps.B, bt.n, 0, x, centre, s, G)
            finite[len(plan)] = torch.isfinite(x[:bt.n]).all()     # bookkeeping for the refusal below; it stays on the device
            plan.append((bt.row0, bt.n))
    finally:
        feed.close()
    c_h, s_h, G_h, fin = centre.cpu().numpy(), s.cpu().numpy(), G.cpu().numpy(), finite.cpu().numpy()      # the one read of the accumulators
    if not fin.all() or not (np.all(np.isfinite(s_h)) and np.all(np.isfinite(np.triu(G_h)))):
        k = int(np.flatnonzero(~fin)[0]) if not fin.all() else None
        where = ("first among the images in rows [%d, %d)" % (plan[k][0], plan[k][0] + plan[k][1])) if k is not None else "the sums overflowed"
        raise ValueError("%s: the feature statistics are not finite (%s): a NaN or infinite activation" % (who, where))
    mean, cov, rho, W = settle(c_h, s_h, G_h, N, shrink, who)
    dom = Domain(N, grid, geo, c_h, mean, cov, rho, W)
    if holdout is not None:
        hids = list(holdout.image_ids)
        if len(hids) < 1:
            raise ValueError("%s: the holdout dataset has no images" % who)
        dp = DomainPass(ps, len(hids), dom)
        feed = EvalFeeder(model, holdout, ps.cfg, workers=loader_workers(ps.cfg, workers), labels=False, cache=cache)
        try:
            for bt in feed:
                ps.run(bt.images)
                dp.launch(bt.n, bt.row0)
        finally:
            feed.close()
        scores = dp.table(len(hids))[:, SCORE]
        if not np.all(np.isfinite(scores)):
            raise ValueError("%s: %d of %d holdout images have a score that is not finite" % (who, int(np.sum(~np.isfinite(scores))), len(hids)))
        dom.holdout_scores = np.sort(scores)
    return dom
