"""urso_quat_gmm_fit without a GPU: the premises of the golden fixture (tests/golden/ori_gmm.npz, made by make_gmm_golden.py from
the reference's own pose_estimator.fit_GMM_to_orientation) and the argument checks of the entry point, which run before any launch."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ori_gmm.npz")


def _gold():
    return np.load(GOLD)


def test_gmm_fixture_maps_match_orientation_codec():
    from ursonet_amd.pose import OrientationCodec
    g = _gold()
    ns = sorted({int(g[c + "/n"]) for c in g["cases"]})
    assert 32 in ns and {8, 16, 24} <= set(ns)
    for n in ns:
        hq = OrientationCodec(n, float(g["beta"])).H_quat
        assert hashlib.sha256(np.ascontiguousarray(hq).tobytes()).hexdigest() == str(g["map_sha256_n%d" % n]), n


def test_gmm_fixture_margins_clear_the_floors():
    """Every discrete decision of every case (model acceptance, initial-mean masking, initial-mean choice) is further from
    its threshold than fp32 evaluation can move it."""
    g = _gold()
    score_floor, dist_floor, gap_floor = g["floors"]
    assert len(g["cases"]) >= 12
    for c in g["cases"]:
        m = len(g[c + "/scores"])
        nmax = int(g[c + "/nr_max_modes"])
        sm = g[c + "/score_margin"]
        assert m >= 1, c
        assert np.all(np.abs(sm) > score_floor), (c, sm)
        assert np.all(sm[:m - 1] > 0) and (m == nmax - 1 or sm[m - 1] < 0), (c, sm)   # accepted, then the rejection
        ran = min(len(sm) + 1, nmax - 1)
        assert g[c + "/dist_margin"][:ran].min() > dist_floor, c
        assert g[c + "/pmf_gap"][:ran].min() > gap_floor, c
        assert g[c + "/mean"].shape == (m, 4) and g[c + "/var_out"].shape == (m,) and g[c + "/prior"].shape == (m,)
        assert np.all(np.diff(g[c + "/prior"]) <= 0), c                                  # sorted by prior


def test_gmm_fixture_covers_the_issue_cases():
    g = _gold()
    modes = {str(c): len(g[c + "/scores"]) for c in g["cases"]}
    assert modes["single_n8"] == modes["single_n16"] == modes["single_n24"] == 1
    assert modes["pair180_n16"] == modes["pair180_n24"] == 2
    assert modes["pair90_n24"] == 2 and modes["pair90_n16"] == 1
    assert any(c.startswith("logits_") for c in modes) and "maxmodes5_n24" in modes
    assert {int(g[c + "/nr_iterations"]) for c in g["cases"]} >= {1, 3, 5}


def _fit(hip, **kw):
    a = dict(B=2, K=64, in_d=0x1000, in_is_pmf=1, hquat_d=0x2000, var=0.01, nr_iterations=5, nr_max_modes=4,
             mean_d=0x3000, var_d=0x4000, prior_d=0x5000, score_d=0x6000, nmodes_d=0x7000)
    a.update(kw)
    f = hip._lib.urso_quat_gmm_fit
    return f(a["B"], a["K"], a["in_d"], a["in_is_pmf"], a["hquat_d"], ctypes.c_float(a["var"]), a["nr_iterations"],
             a["nr_max_modes"], a["mean_d"], a["var_d"], a["prior_d"], a["score_d"], a["nmodes_d"], None)


@pytest.mark.parametrize("bad,needle", [
    (dict(in_d=None), "null"), (dict(hquat_d=None), "null"), (dict(mean_d=None), "null"), (dict(var_d=None), "null"),
    (dict(prior_d=None), "null"), (dict(score_d=None), "null"), (dict(nmodes_d=None), "null"),
    (dict(B=0), "positive"), (dict(K=-1), "positive"), (dict(hquat_d=0x2004), "aligned"),
    (dict(var=0.0), "var"), (dict(var=-1.0), "var"), (dict(var=float("inf")), "var"), (dict(var=float("nan")), "var"),
    (dict(nr_iterations=0), "nr_iterations"), (dict(nr_max_modes=1), "nr_max_modes"), (dict(nr_max_modes=6), "nr_max_modes"),
])
def test_quat_gmm_fit_refuses_bad_arguments(bad, needle):
    import ursonet_amd.hip as hip
    rc = _fit(hip, **bad)
    assert rc == -1 and needle in hip.last_error() and "urso_quat_gmm_fit" in hip.last_error(), (rc, hip.last_error())


def test_mode_errors_marks_slots_past_n_modes():
    from ursonet_amd.pose import mode_errors
    q = np.array([[0, 0, 0, 1.0], [0, 0, np.sin(np.pi / 4), np.cos(np.pi / 4)], [0, 0, 0, 0]], dtype=np.float32)
    e = mode_errors(q[None], [2], np.array([0, 0, 0, 1.0]))
    assert e.shape == (1, 3) and np.isnan(e[0, 2])
    assert np.allclose(e[0, :2], [0.0, 90.0], atol=1e-3)
