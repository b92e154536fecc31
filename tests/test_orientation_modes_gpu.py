"""urso_quat_gmm_fit (ursonet_amd.pose.fit_orientation_modes / fit_GMM_to_orientation) on the MI355X against the reference's own
pose_estimator.fit_GMM_to_orientation (tests/golden/ori_gmm.npz, made by tests/golden/make_gmm_golden.py), plus properties the
fixture cannot show: logits against host-softmaxed PMFs, batch invariance, K = 262,144, tied and uniform PMFs."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ori_gmm.npz")
# Gates, about three times the largest deviation measured on an MI355X over every fixture case (PMF and logit inputs):
# 1 - |dot| 3.9e-8, prior 1.6e-7, variance 9.3e-6 relative, score 2.2e-6.
DOT_GATE, PRIOR_GATE, VAR_GATE, SCORE_GATE = 1.5e-7, 5e-7, 3e-5, 7e-6

_maps = {}


def _map(n, beta=6.0):
    from ursonet_amd.pose import OrientationCodec
    if (n, beta) not in _maps:
        _maps[(n, beta)] = OrientationCodec(n, beta)
    return _maps[(n, beta)]


def _rot_z(q, deg):
    h = np.deg2rad(deg) / 2
    x1, y1, z1, w1 = 0.0, 0.0, np.sin(h), np.cos(h)
    x2, y2, z2, w2 = q
    return np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])


def _deviations(mean, var, prior, score, m, rm, rv, rp, rs):
    """(1 - min |dot|, max |prior diff|, max relative var diff, max |score diff|) over the m accepted modes."""
    return (float(1 - np.abs((mean[:m].astype(np.float64) * rm).sum(-1)).min()), float(np.abs(prior[:m] - rp).max()),
            float((np.abs(var[:m] - rv) / np.abs(rv)).max()), float(np.abs(score[:m] - rs).max()))


def _check(dev, what):
    assert dev[0] <= DOT_GATE and dev[1] <= PRIOR_GATE and dev[2] <= VAR_GATE and dev[3] <= SCORE_GATE, (what, dev)


def test_parity_with_reference_fixture():
    """Every fixture case, as a PMF and (where the case has them) as logits: n_modes exact; means, priors (absolute),
    variances (relative) and scores (absolute) within the gates above.  Measured: 1 - |dot| <= 3.9e-8, prior 1.6e-7,
    variance 9.3e-6, score 2.2e-6."""
    from ursonet_amd.pose import fit_orientation_modes
    g = np.load(GOLD)
    worst = np.zeros(4)
    for c in g["cases"]:
        n, var = int(g[c + "/n"]), float(g[c + "/var"])
        nit, nmax = int(g[c + "/nr_iterations"]), int(g[c + "/nr_max_modes"])
        rm, rv, rp, rs = g[c + "/mean"], g[c + "/var_out"], g[c + "/prior"], g[c + "/scores"]
        inputs = [(g[c + "/pmf"], True)] + ([(g[c + "/logits"], False)] if c + "/logits" in g else [])
        for x, is_pmf in inputs:
            mean, v, pri, sc, nm = fit_orientation_modes(x[None], _map(n).H_quat, var, nit, nmax, pmf=is_pmf)
            m = len(rs)
            assert nm[0] == m, (c, is_pmf, nm[0], m)
            assert np.all(np.isnan(sc[0, m:])) and np.all(pri[0, m:] == 0) and np.all(mean[0, m:] == 0)
            dev = _deviations(mean[0], v[0], pri[0], sc[0], m, rm, rv, rp, rs)
            _check(dev, (c, is_pmf))
            worst = np.maximum(worst, dev)
    print("\nGMM parity, largest deviations: 1-|dot| %.3g  prior %.3g  var(rel) %.3g  score %.3g" % tuple(worst))


def test_logits_equal_host_softmaxed_pmf():
    from ursonet_amd.pose import fit_orientation_modes, stable_softmax
    rng = np.random.default_rng(7)
    c = _map(16)
    q1 = rng.normal(size=4); q1 /= np.linalg.norm(q1)
    z = np.stack([rng.normal(scale=0.3, size=len(c.H_quat)) + a * np.exp(-((2 * np.arccos(np.minimum(1, np.abs(c.H_quat @ q))) / np.pi) ** 2)
                                                                          / (8 * c.var))
                  for q, a in ((q1, 6.0), (_rot_z(q1, 180), 5.0), (_rot_z(q1, 90), 4.0))]).astype(np.float32)
    z[2] += 4.0 * np.exp(-((2 * np.arccos(np.minimum(1, np.abs(c.H_quat @ q1))) / np.pi) ** 2) / (8 * c.var)).astype(np.float32)
    pm = np.stack([stable_softmax(r) for r in z]).astype(np.float32)
    a = fit_orientation_modes(z, c.H_quat, c.var)
    b = fit_orientation_modes(pm, c.H_quat, c.var, pmf=True)
    assert np.array_equal(a[4], b[4]), (a[4], b[4])
    for i in range(len(z)):
        m = int(a[4][i])
        dev = _deviations(a[0][i], a[1][i], a[2][i], a[3][i], m, b[0][i, :m], b[1][i, :m], b[2][i, :m], b[3][i, :m])
        print("\nlogits vs host softmax, image %d (%d modes): 1-|dot| %.3g  prior %.3g  var(rel) %.3g  score %.3g" % ((i, m) + dev))
        _check(dev, i)


def test_batch_of_37_equals_each_fit_alone_bit_for_bit():
    from ursonet_amd.pose import fit_orientation_modes
    rng = np.random.default_rng(11)
    c = _map(24)
    pm = []
    for i in range(37):
        k = 1 + i % 3
        qs = rng.normal(size=(k, 4))
        w = rng.uniform(0.2, 1.0, size=k)
        pm.append((w[:, None] * c.encode(qs)).sum(0) / w.sum())
    pm = np.stack(pm).astype(np.float32)
    allb = fit_orientation_modes(pm, c.H_quat, c.var, pmf=True)
    assert len(set(allb[4].tolist())) >= 2
    for i in range(len(pm)):
        one = fit_orientation_modes(pm[i:i + 1], c.H_quat, c.var, pmf=True)
        for a, b in zip(allb, one):
            assert a[i:i + 1].tobytes() == b.tobytes(), i


@pytest.mark.parametrize("planted", [2, 3])
def test_n64_planted_modes(planted):
    """K = 262,144 (the n = 64 released weights): planted poses 120 / 180 degrees apart, weights >= 0.2."""
    from ursonet_amd.pose import fit_orientation_modes
    rng = np.random.default_rng(64 + planted)
    c = _map(64)
    q1 = rng.normal(size=4); q1 /= np.linalg.norm(q1)
    if planted == 2:
        qs, w = np.stack([q1, _rot_z(q1, 180)]), np.array([0.62, 0.38])
    else:
        qs, w = np.stack([q1, _rot_z(q1, 120), _rot_z(q1, 240)]), np.array([0.45, 0.33, 0.22])
    pm = (w[:, None] * c.encode(qs).astype(np.float64)).sum(0).astype(np.float32)
    mean, v, pri, sc, nm = fit_orientation_modes(pm[None], c.H_quat, c.var, pmf=True)
    m = int(nm[0])
    assert m == planted, (m, pri)
    assert np.all(np.isfinite(mean[0, :m])) and np.all(np.isfinite(v[0, :m])) and np.all(np.isfinite(sc[0, :m]))
    ang = 2 * np.degrees(np.arccos(np.minimum(1, np.abs(mean[0, :m].astype(np.float64) @ qs.T))))       # [mode, planted]
    bin_width = 360.0 / (64 - 1)
    assert np.all(ang.min(axis=0) < bin_width), ang
    order = ang.argmin(axis=1)                      # planted pose of each mode
    assert sorted(order.tolist()) == list(range(planted))
    assert np.abs(pri[0, :m] - w[order]).max() < 0.02, (pri[0, :m], w[order])


def test_uniform_and_tied_pmfs_are_deterministic_and_finite():
    from ursonet_amd.pose import fit_orientation_modes
    c = _map(16)
    K = len(c.H_quat)
    rng = np.random.default_rng(3)
    uni = np.full((1, K), 1.0 / K, np.float32)
    relu = (np.maximum(rng.normal(size=(2, K)), 0) * 3).astype(np.float32)          # about half the bins tied at logit 0
    for x, is_pmf in ((uni, True), (relu, False)):
        a = fit_orientation_modes(x, c.H_quat, c.var, pmf=is_pmf)
        b = fit_orientation_modes(x, c.H_quat, c.var, pmf=is_pmf)
        for u, w in zip(a, b):
            assert u.tobytes() == w.tobytes()
        for i in range(len(x)):
            m = int(a[4][i])
            assert m >= 1
            for arr in a[:4]:
                assert np.all(np.isfinite(arr[i, :m]))


def test_drop_in_matches_reference_types_and_batched_form():
    from ursonet_amd.pose import fit_orientation_modes
    from ursonet_amd.utils import fit_GMM_to_orientation
    g = np.load(GOLD)
    c = "pair180_n24"
    n, var = int(g[c + "/n"]), float(g[c + "/var"])
    pm = g[c + "/pmf"]
    Qm, Qv, Qp, sc = fit_GMM_to_orientation(_map(n).H_quat, pm, 5, var)
    dts = [str(d) for d in g[c + "/dtypes"]]
    m = len(g[c + "/scores"])
    assert isinstance(sc, list) and len(sc) == m
    assert Qm.shape == (m, 4) and Qv.shape == (m,) and Qp.shape == (m,)
    assert [str(Qm.dtype), str(Qv.dtype), str(Qp.dtype), str(np.asarray(sc[0]).dtype)] == dts
    mean, v, pri, s, nm = fit_orientation_modes(pm[None], _map(n).H_quat, var, 5, 4, pmf=True)
    assert nm[0] == m and np.array_equal(Qm, mean[0, :m]) and np.array_equal(Qv, v[0, :m]) and np.array_equal(Qp, pri[0, :m])
    assert np.array_equal(np.asarray(sc, dtype=np.float32), s[0, :m])


def test_mode_errors_against_host_numpy():
    from ursonet_amd.pose import fit_orientation_modes, mode_errors
    g = np.load(GOLD)
    cs = ["pair180_n16", "pair90_n24", "single_n16"]
    out = []
    for c in cs:
        nn = int(g[c + "/n"])
        out.append(fit_orientation_modes(g[c + "/pmf"][None], _map(nn).H_quat, float(g[c + "/var"]), pmf=True))
    rng = np.random.default_rng(5)
    qgt = rng.normal(size=(len(cs), 4)); qgt /= np.linalg.norm(qgt, axis=1, keepdims=True)
    mean = np.concatenate([o[0] for o in out]); nm = np.concatenate([o[4] for o in out])
    e = mode_errors(mean, nm, qgt)
    assert e.shape == (len(cs), 3)
    for i in range(len(cs)):
        for k in range(3):
            if k < nm[i]:
                d = min(1.0, abs(float(np.dot(mean[i, k].astype(np.float64), qgt[i]))))
                assert abs(e[i, k] - np.degrees(2 * np.arccos(d))) < 1e-9
            else:
                assert np.isnan(e[i, k])
