#!/usr/bin/env python3
"""Golden fits of multimodal orientation PMFs by CALLING the reference's own pose_estimator.fit_GMM_to_orientation.

Runs only in the build container (needs /root/reference); tests/golden/ori_gmm.npz is committed and is the only thing that
travels.  pose_estimator imports TensorFlow / Keras / the dataset modules at module scope; the function called here never
touches them, so empty stub modules are injected (as make_golden.py does for utils).

Stored per case: the PMF (and the logits it came from, where there are any), n, var, nr_iterations, nr_max_modes and the
reference's outputs.  The bin maps are not stored: tests rebuild them with ursonet_amd.pose.OrientationCodec(n, BETA) and
check them against the SHA-256 stored here.  Every case also carries the margins of its discrete decisions, from a float64
mirror of the fit that records the score of every model size, rejected ones included:
  score_margin  score_N - (score_last_accepted + 0.005) for every model size that ran (> 0 accepted, < 0 the rejection);
  dist_margin   per initial pick: how far the d^2 < 9 var masking tests that decide it are from the threshold;
  pmf_gap       per initial pick: its PMF minus the next eligible bin's, relative to its own.
A case whose margins fall under the floors below is dropped.

    python tests/golden/make_gmm_golden.py
"""
import contextlib
import hashlib
import io
import os
import sys
import time
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
BETA = 6.0
SCORE_FLOOR, DIST_FLOOR, GAP_FLOOR = 1e-3, 1e-5, 1e-4


def import_reference():
    for n in ["tensorflow", "keras", "net", "urso", "speed", "cv2", "skimage", "skimage.color", "skimage.io", "skimage.transform"]:
        if n not in sys.modules:
            sys.modules[n] = types.ModuleType(n)
    for sub in ("color", "io", "transform"):
        setattr(sys.modules["skimage"], sub, sys.modules["skimage." + sub])
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, REF)
    import pose_estimator  # noqa
    import utils  # noqa
    return pose_estimator, utils


def d2(q, m):
    """Squared normalised angular distance, float64: [K] x [4] -> [K]."""
    c = np.clip(np.abs(q.astype(np.float64) @ np.asarray(m, dtype=np.float64)), 0.0, 1.0)
    return (2 * np.arccos(c) / np.pi) ** 2


def greedy_picks(q, pmf, var, M):
    """Initial means of pose_estimator.py:60-79 (ties to the lowest bin index) and the margins of each pick."""
    pmf = pmf.astype(np.float64)
    picks, dist_m, gaps = [], [], []
    dd = []                                   # d^2 to each previous pick
    for k in range(M):
        excl = np.zeros(len(pmf), bool)
        for j, p in enumerate(picks):
            excl |= dd[j] < 9 * var
            excl[p] = True
        elig = np.flatnonzero(~excl)
        if len(elig) == 0:
            picks.append(-1); dist_m.append(np.inf); gaps.append(np.inf)
            continue
        order = elig[np.argsort(-pmf[elig], kind="stable")]
        p = int(order[0])
        nxt = pmf[order[1]] if len(order) > 1 else 0.0
        gaps.append((pmf[p] - nxt) / pmf[p] if pmf[p] > 0 else 0.0)
        # margins: the pick is clear of every previous pick's ball, every higher-PMF bin is inside one of them
        m = np.inf
        if dd:
            D = np.stack(dd)                                  # [k, K]
            m = min(m, float((D[:, p] - 9 * var).min()))
            higher = np.flatnonzero(pmf > pmf[p])
            higher = higher[~np.isin(higher, picks)]
            if len(higher):
                m = min(m, float((9 * var - D[:, higher]).max(axis=0).min()))
        dist_m.append(m)
        picks.append(p)
        dd.append(d2(q, q[p]))
    return picks, np.array(dist_m), np.array(gaps)


def mirror_scores(q, pmf, var, nit, M, picks):
    """float64 mirror of the EM loop: the score of every model size 1..M (no early stop)."""
    pmf = pmf.astype(np.float64)
    qd = q.astype(np.float64)
    out = []
    for N in range(1, M + 1):
        mu = np.stack([qd[p] if p >= 0 else np.zeros(4) for p in picks[:N]])
        v = np.full(N, var); pri = np.full(N, 1.0 / N)
        for it in range(nit):
            D = np.stack([d2(q, m) for m in mu], axis=1)
            pk = 1e-18 + np.exp(-D / (2 * v)) / np.sqrt(2 * np.pi * v)
            pp = pk * pri
            pX = pp.sum(1)
            W = pp / pX[:, None] * pmf[:, None]
            Z = W.sum(0)
            for k in range(N):
                A = (qd * (W[:, k] / Z[k])[:, None]).T @ qd
                s, V = np.linalg.eigh(A)
                mu[k] = V[:, -1]
                v[k] = (W[:, k] / Z[k] * d2(q, mu[k])).sum()
            pri = Z
            if N == 1 and it == 1:
                break
        out.append(float((pmf * np.log(pX)).sum()))
    return out


def score_margins(scores):
    acc, m = [scores[0]], []
    for s in scores[1:]:
        m.append(s - (acc[-1] + 0.005))
        if m[-1] > 0:
            acc.append(s)
        else:
            break
    return np.array(m)


def rot_z(q, deg):
    """q turned by `deg` degrees about z (left-multiplied), quaternions (x, y, z, w)."""
    h = np.deg2rad(deg) / 2
    r = np.array([0, 0, np.sin(h), np.cos(h)])
    x1, y1, z1, w1 = r
    x2, y2, z2, w2 = q
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def main():
    sys.path.insert(0, ROOT)
    from ursonet_amd.pose import OrientationCodec
    pe, utils = import_reference()
    rng = np.random.default_rng(20261016)

    def rq():
        q = rng.normal(size=4)
        return q / np.linalg.norm(q)

    codecs = {}

    def codec(n):
        if n not in codecs:
            codecs[n] = OrientationCodec(n, BETA)
        return codecs[n]

    def mix(n, qs, ws):
        c = codec(n)
        return sum(w * c.encode(q)[0].astype(np.float64) for q, w in zip(qs, ws)).astype(np.float32)

    def planted_logits(n, qs, amps):
        c = codec(n)
        z = rng.normal(scale=0.3, size=len(c.H_quat))
        for q, a in zip(qs, amps):
            z += a * np.exp(-d2(c.H_quat, q) / (2 * 4 * c.var))
        return z.astype(np.float32)

    cases = []       # (name, n, pmf, logits or None, nit, nmax)
    q1 = rq()
    for n in (8, 16, 24):
        cases.append(("single_n%d" % n, n, codec(n).encode(rq())[0], None, 5, 4))
    for n in (16, 24):
        cases.append(("pair180_n%d" % n, n, mix(n, [q1, rot_z(q1, 180)], [0.6, 0.4]), None, 5, 4))
        cases.append(("pair90_n%d" % n, n, mix(n, [q1, rot_z(q1, 90)], [0.6, 0.4]), None, 5, 4))
    qa, qb, qc = rq(), rq(), rq()
    cases.append(("triple_n16", 16, mix(16, [qa, qb, qc], [0.45, 0.33, 0.22]), None, 5, 4))
    cases.append(("triple_n24", 24, mix(24, [qa, qb, qc], [0.45, 0.33, 0.22]), None, 5, 4))
    for n in (8, 16, 24):
        z = planted_logits(n, [rq(), rq()], [6.0, 5.5])
        cases.append(("logits_n%d" % n, n, utils.stable_softmax(z), z, 5, 4))
    cases.append(("pair180_n32", 32, mix(32, [q1, rot_z(q1, 180)], [0.6, 0.4]), None, 5, 4))
    cases.append(("iters1_n16", 16, mix(16, [qa, qb], [0.6, 0.4]), None, 1, 4))
    cases.append(("iters3_n16", 16, mix(16, [qa, qb], [0.6, 0.4]), None, 3, 4))
    cases.append(("maxmodes5_n24", 24, mix(24, [qa, qb, qc, rq()], [0.3, 0.27, 0.23, 0.2]), None, 5, 5))

    store = {"numpy_version": np.array(np.__version__), "beta": np.array(BETA)}
    for n in sorted({c[1] for c in cases}):
        store["map_sha256_n%d" % n] = np.array(hashlib.sha256(np.ascontiguousarray(codec(n).H_quat).tobytes()).hexdigest())
    kept = []
    for name, n, pmf, logits, nit, nmax in cases:
        c = codec(n)
        var = (BETA / n) ** 2 / 12                                        # pose_estimator.py:333-334
        t0 = time.time()
        with contextlib.redirect_stdout(io.StringIO()):
            Qm, Qv, Qp, sc = pe.fit_GMM_to_orientation(c.H_quat, pmf, nit, var, nmax)
        dt = time.time() - t0
        Qm = np.asarray(Qm).copy()
        for k in range(len(Qm)):                                           # sign as urso_quat_wavg_decode
            if Qm[k, np.argmax(np.abs(Qm[k]))] < 0:
                Qm[k] = -Qm[k]
        picks, dm, gaps = greedy_picks(c.H_quat, pmf, var, nmax - 1)
        allsc = mirror_scores(c.H_quat, pmf, var, nit, nmax - 1, picks)
        sm = score_margins(allsc)
        m = len(sc)
        # decisions that matter: the picks of every model that ran, and the scores that decided
        ran = min(len(sm) + 1, nmax - 1)
        ok = (np.abs(sm).min() if len(sm) else np.inf) > SCORE_FLOOR and dm[:ran].min() > DIST_FLOOR and gaps[:ran].min() > GAP_FLOOR
        ok = ok and np.allclose(allsc[:m], np.asarray(sc, dtype=np.float64), atol=1e-3) and len(sm) >= min(m, nmax - 2)
        print("%-14s n=%2d modes=%d  %.2fs  score margins %s  dist %s  gap %s  %s"
              % (name, n, m, dt, np.round(sm, 4), np.round(dm[:ran], 5), np.round(gaps[:ran], 5), "ok" if ok else "DROPPED"))
        if not ok:
            continue
        kept.append(name)
        p = name + "/"
        store[p + "n"] = np.array(n); store[p + "var"] = np.array(var)
        store[p + "nr_iterations"] = np.array(nit); store[p + "nr_max_modes"] = np.array(nmax)
        store[p + "pmf"] = np.asarray(pmf, dtype=np.float32)
        if logits is not None:
            store[p + "logits"] = logits
        store[p + "mean"] = Qm; store[p + "var_out"] = np.asarray(Qv); store[p + "prior"] = np.asarray(Qp)
        store[p + "scores"] = np.asarray(sc)
        store[p + "dtypes"] = np.array([str(np.asarray(Qm).dtype), str(np.asarray(Qv).dtype), str(np.asarray(Qp).dtype),
                                        str(np.asarray(sc[0]).dtype)])
        store[p + "score_margin"] = sm; store[p + "dist_margin"] = dm; store[p + "pmf_gap"] = gaps
    store["cases"] = np.array(kept)
    store["floors"] = np.array([SCORE_FLOOR, DIST_FLOOR, GAP_FLOOR])
    np.savez_compressed(os.path.join(OUT, "ori_gmm.npz"), **store)
    print("wrote ori_gmm.npz: %d cases" % len(kept))


if __name__ == "__main__":
    main()
