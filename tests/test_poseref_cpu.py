"""tests/poseref.py proven on the CPU before it judges a kernel (the pattern of tests/test_inputref_cpu.py):

* the references against what the project already trusts -- oracle/pose_math.py and the goldens recorded from the reference's own modules
  (ori_codec.npz, eval.npz, se3lib_basic.npz).  Where a golden is fp32 the bound is the golden's OWN rounding, stated in the test; every
  measured value is printed;
* the case generators' conditions: every so3_to_quat branch is taken, and the rows a gap condition excludes stay within the caps that
  tests/test_pose_decode_exact_gpu.py relies on (the "reference alone" check of every cap);
* the gates on an fp32 emulation of quat_wavg_kernel (poseref.emulate_wavg): the faithful emulation is ACCEPTED at every K of the GPU test,
  and the same emulation with one mistake injected is REJECTED, one mistake at a time.

Needs no GPU and imports nothing that loads the HIP library."""
import os

import numpy as np
import pytest

import poseref as R
from oracle import pose_math as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U32 = 2.0 ** -24                                                    # unit roundoff of fp32


def _pm(a, b):
    """max over rows of min(|a - b|, |a + b|): quaternions / eigenvectors compared up to sign."""
    a, b = np.atleast_2d(a).astype(np.float64), np.atleast_2d(b).astype(np.float64)
    return float(np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)).max())


# ------------------------------------------------------------------------------------------------ pins
def test_conversions_against_oracle_and_se3lib_golden():
    g = np.load(os.path.join(GOLD, "se3lib_basic.npz"))
    # float64 goldens of the same formulas: a few ulp of O(1) values
    d_R = max(np.abs(R.euler_to_so3(*e) - r).max() for e, r in zip(g["eul"], g["e2R"]))
    d_q = max(np.abs(R.so3_to_quat(r)[0] - q).max() for r, q in zip(g["e2R"], g["R2q"]))
    d_q2R = max(np.abs(R.quat_to_so3(q) - r).max() for q, r in zip(g["qs"], g["q2R"]))
    d_rt = max(np.abs(R.quat_to_so3(R.so3_to_quat(r)[0]) - r).max() for r in g["e2R"])
    print("euler_to_so3 %.2e  so3_to_quat %.2e  quat_to_so3 %.2e  round trip %.2e" % (d_R, d_q, d_q2R, d_rt))
    assert max(d_R, d_q, d_q2R) <= 4 * 2.0 ** -52 and d_rt <= 16 * 2.0 ** -52
    # the oracle's functions on the Euler cases of the GPU test, every branch
    e = R.euler_cases().astype(np.float64)
    worst = 0.0
    for x in e:
        Rm = R.euler_to_so3(*x)
        worst = max(worst, np.abs(Rm - P.euler2SO3_left(*x)).max(), np.abs(R.so3_to_quat(Rm)[0] - np.asarray(P.SO32quat(Rm))).max())
    print("vs oracle on euler_cases: %.2e" % worst)
    assert worst <= 4 * 2.0 ** -52
    # keypoint encoding
    q, c = R.random_quats(np.random.default_rng(0), 8), np.random.default_rng(1).uniform(-5, 20, (8, 3))
    for qi, ci in zip(q, c):
        k1, k2 = P.encode_as_keypoints(qi, ci)
        r1, r2 = R.encode_as_keypoints(qi, ci)
        assert np.abs(r1 - k1.ravel()).max() <= 1e-14 and np.abs(r2 - k2.ravel()).max() <= 1e-14


def test_regressed_heads_against_eval_golden():
    """q_ref of eval.npz is the reference's own float64 decode of the recorded fp32 outputs: euler, angle-axis, keypoints (its SVD)."""
    g = np.load(os.path.join(GOLD, "eval.npz"))
    d_e = _pm(np.array([R.so3_to_quat(R.euler_to_so3(*x.astype(np.float64)))[0] for x in g["euler/ori"]]), g["euler/q_ref"])
    d_a = _pm(np.array([R.angle_axis_to_quat(v) for v in g["angle_axis/ori"]]), g["angle_axis/q_ref"])
    k = np.array([R.keypoints_to_quat(a, b, c) for a, b, c in zip(g["keypoints/ori"], g["keypoints/ori2"], g["keypoints/loc"])])
    d_k = _pm(k, g["keypoints/q_ref"])
    print("euler %.2e  angle-axis %.2e  keypoints %.2e" % (d_e, d_a, d_k))
    assert d_e <= 1e-14 and d_a <= 1e-14 and d_k <= 1e-12       # the SVD's vectors are conditioned by the singular-value gap (~1), not by ulp


def test_scatter_and_top_vector_against_wavg_golden():
    """wavg_A_* is the reference's A accumulated in FLOAT32 in bin order from float64 weights: K sequential fp32 additions of float64
    products, so |A_gold - A| <= K u M (u = 2^-24, M = sum w |h_i h_j|).  Rows 4.. are softmaxes of logits_*, which the reference computes
    in fp32: three more roundings per weight.  wavg_q_* is np.linalg.eig of that fp32 A, which LAPACK solves in SINGLE precision (sgeev:
    backward error of a few n u |A|, |A| <= 1), so against top_vector of the same matrix the bound is 16 u / gap."""
    g = np.load(os.path.join(GOLD, "ori_codec.npz"))
    for n in (8, 16):
        hq, w = g["Hquat_%d" % n], g["wavg_w_%d" % n]
        K = len(hq)
        A = R.pmf_scatter(w, hq)
        Mabs = (w @ np.abs((hq.astype(np.float64)[:, :, None] * hq.astype(np.float64)[:, None, :]).reshape(K, 16))).reshape(-1, 4, 4)
        r1 = (np.abs(g["wavg_A_%d" % n] - A) / (K * U32 * Mabs)).max()
        A2, M2 = R.scatter(g["logits_%d" % n], hq)
        r2 = (np.abs(g["wavg_A_%d" % n][4:] - A2) / ((K + 3) * U32 * M2)).max()
        v, gap, _ = R.top_vector(g["wavg_A_%d" % n].astype(np.float64))
        dv = np.minimum(np.linalg.norm(v - g["wavg_q_%d" % n], axis=1), np.linalg.norm(v + g["wavg_q_%d" % n], axis=1))
        r3 = (dv / (16 * U32 / gap)).max()
        print("n=%d: A (weights) %.3f of K u M, A (logits) %.3f, eigenvector %.3f of 16 u / gap (min gap %.2e)" % (n, r1, r2, r3, gap.min()))
        assert r1 <= 1 and r2 <= 1 and r3 <= 1
    # the oracle's own loop on a small map
    hq, w = g["Hquat_4"], g["fast_4"]
    for wi in w[:3]:
        q, A32 = P.quat_weighted_avg(hq, wi)
        A = R.pmf_scatter(wi[None], hq)[0]
        assert np.abs(A32 - A).max() <= 64 * U32
        assert _pm(R.top_vector(A32.astype(np.float64))[0], q) <= 16 * U32 / R.top_vector(A32.astype(np.float64))[1]


def test_existing_soft_gates_against_the_fp32_golden():
    """How far the fp32 golden q of the soft head (eval.npz q_ref, ori_codec wavg_q) lies from the float64 decode of the same logits: this
    is what the two existing gates (1 - 1e-5 in the normalised dot product, 0.51 degree) really have to allow.  The golden lies within
    1 - dot <= 1e-11 (asserted; 4e-6 rad measured) and the kernel's arithmetic within 3e-4 degree = 5e-6 rad of the float64 decode
    (test_emulation_passes_every_gate...), together 1e-5 rad or 1 - dot = 1.3e-11: the two gates are tightened to 1 - 1e-9 (9e-5 rad), a
    margin of 9 in the angle and 80 in the dot product."""
    g, gc = np.load(os.path.join(GOLD, "eval.npz")), np.load(os.path.join(GOLD, "ori_codec.npz"))
    from ursonet_amd.pose import OrientationCodec
    for c in ("soft_n8", "soft_n16"):
        hq = OrientationCodec(int(g[c + "/ori_bins"]), float(g["beta"])).H_quat
        A, M = R.scatter(g[c + "/ori"], hq)
        v, gap, _ = R.top_vector(A)
        ang = R.angle(v, g[c + "/q_ref"])
        bound = 2 * np.arcsin(np.minimum(1, len(hq) * U32 * np.linalg.norm(M.reshape(-1, 16), axis=1) / gap)) + 2.0 ** -21
        print(c, "golden q vs float64 decode: max %.2e rad (1 - dot %.1e), K u |M|_F / gap bound %.2e" % (ang.max(), 1 - np.cos(ang.max() / 2), bound.max()))
        assert np.all(ang <= bound) and 1 - np.cos(ang.max() / 2) <= 1e-11
        # encoded target: q_enc_ref is fp32
        ve, gape, _ = R.top_vector(R.pmf_scatter(g[c + "/enc_ori"], hq))
        print(c, "golden q_enc vs float64: %.2e rad" % R.angle(ve, g[c + "/q_enc_ref"]).max())
        assert np.all(R.angle(ve, g[c + "/q_enc_ref"]) <= 2 * np.arcsin(np.minimum(1, len(hq) * U32 / gape)) + 2.0 ** -21)
    for n in (8, 16):
        A, _ = R.scatter(gc["logits_%d" % n], gc["Hquat_%d" % n])
        ang = R.angle(R.top_vector(A)[0], gc["wavg_q_%d" % n][4:])
        print("ori_codec n=%d golden q vs float64: %.2e rad" % (n, ang.max()))
        assert 1 - np.cos(ang.max() / 2) <= 1e-11
        assert R.angle(R.emulate_wavg(gc["logits_%d" % n], gc["Hquat_%d" % n])[0], gc["wavg_q_%d" % n][4:]).max() <= 1e-5


def test_location_helpers_against_oracle_and_golden():
    from ursonet_amd.pose import location_map
    g = np.load(os.path.join(GOLD, "eval.npz"))
    mx, mn = g["loc_class/loc_lims"]
    lm = location_map(int(g["loc_class/loc_bins"]), mx, mn)
    z = g["loc_class/loc"].astype(np.float32)
    est, pk = R.loc_softmax(z, lm)
    ora = np.array([P.decode_location_classified(r.astype(np.float64), lm) for r in z])
    d1 = np.abs(est - ora).max() / np.abs(lm).max()
    # the golden's loc_ref is the reference's fp32 softmax (K = 512 bins): exp, K-term sum and division in fp32, ~ (K + 3) u relative to max |map|
    d2 = np.abs(est - g["loc_class/loc_ref"]).max() / np.abs(lm).max()
    print("loc_softmax vs oracle (float64) %.2e, vs fp32 golden %.2e of max|map| (bound %.2e)" % (d1, d2, (z.shape[1] + 3) * U32))
    assert d1 <= 1e-14 and d2 <= (z.shape[1] + 3) * U32
    assert np.abs(pk - R.peak(z)).max() == 0
    assert np.abs(pk - np.array([P.stable_softmax(r.astype(np.float64)).max() for r in z])).max() <= 1e-15
    enc = np.linalg.norm(R.first_moment(g["loc_class/enc_loc"], lm) - g["loc_class/loc_gt"], axis=1)
    d3 = (np.abs(enc - g["loc_class/loc_enc_err"]) / g["loc_class/loc_enc_err"]).max()
    print("first_moment -> LOC_ENC_ERR vs golden (float64): %.2e relative" % d3)
    assert d3 <= 1e-10                                                       # a difference of O(10) vectors giving an O(0.1) error: 100 x 1e-15, with margin


# ------------------------------------------------------------------------------------------------ generators
def test_euler_cases_reach_every_branch():
    e = R.euler_cases().astype(np.float64)
    br = np.array([R.so3_to_quat(R.euler_to_so3(*x))[1] for x in e])
    ties = sum(R.so3_branch_margin(R.euler_to_so3(*x)) < 1e-12 for x in e)
    print("rows per branch:", np.bincount(br, minlength=4), "rows within 1e-12 of a branch tie:", ties, "of", len(e))
    assert np.all(np.bincount(br, minlength=4) >= 8)
    assert len(e) == 13 ** 3 + 64 and np.any(np.abs(e[:, 1]) == 90)
    # off the ties every branch still has its 8 rows, so the quaternion comparison (not only the matrix one) sees all four
    off = np.array([R.so3_branch_margin(R.euler_to_so3(*x)) >= 1e-12 for x in e])
    assert np.all(np.bincount(br[off], minlength=4) >= 8)


EMU = {}


def _emulated(K):
    """(z, families, map, A, M, q, a) of the fp32 emulation at K, computed once."""
    if K not in EMU:
        z, fam = R.logit_cases(K, big=K == R.K_BIG)
        hq = R.bin_map(K)
        A, M = R.scatter(z, hq)
        q, a = R.emulate_wavg(z, hq)
        EMU[K] = (z, fam, hq, A, M, q, a)
    return EMU[K]


@pytest.mark.parametrize("K", R.KS + (R.K_BIG,))
def test_emulation_passes_every_gate_and_exclusions_stay_within_caps(K):
    z, fam, hq, A, M, q, a = _emulated(K)
    assert 3 <= len(fam) <= 37
    ra = R.gate_scatter(a, A, M, K)
    rc, low = R.gate_solver(q, a)
    rd, excl = R.gate_decode(q, K, A, M)
    print("K=%d emulation: scatter %.3f  solver %.3f  decode %.3f of the bounds; min gap %.2e" % (K, ra, rc, rd, R.top_vector(A)[1].min()))
    assert ra <= 1 and rc <= 1 and rd <= 1
    # caps: rows below the solver's gap condition only "equal"; rows outside the decode bound only "equal" (and "peak3" at K = 262,144)
    assert {fam[i] for i in np.where(low)[0]} <= {"equal"}
    assert {fam[i] for i in np.where(excl)[0]} <= ({"equal", "peak3"} if K == R.K_BIG else {"equal"})
    _, gap64, _ = R.top_vector(A)
    assert {fam[i] for i in np.where(gap64 < 2e-6)[0]} <= {"equal"}       # the cap of (c) from the reference alone, with a factor 2 for a's own error
    zp, ks = R.planted_cases(K)
    rp = R.gate_planted(R.emulate_wavg(zp, hq)[0], hq[ks])
    za, pairs = R.antipodal_cases(K)
    assert len(pairs) >= (4 if K >= 255 else 0)
    if pairs:
        h = hq.astype(np.float64)
        assert all(h[i] @ h[j] <= -0.5 for i, j in pairs)
        rp = max(rp, R.gate_planted(R.emulate_wavg(za, hq)[0], np.array([h[i] - h[j] for i, j in pairs]) /
                                    np.array([[np.linalg.norm(h[i] - h[j])] for i, j in pairs]), tol=2.0 ** -22))
    print("K=%d emulation: planted %.3f" % (K, rp))
    assert rp <= 1


def test_keypoint_cases_conditions():
    cases, q, exact = R.keypoint_cases()
    assert exact.sum() == 24 and np.sum(np.abs(q[:, 3]) < 1e-12) >= 9 + 8          # 180-degree rotations among the exact and the random poses
    for name, (k1, k2, loc) in cases.items():
        g = np.array([R.horn_gap(a, b, c) for a, b, c in zip(k1, k2, loc)])
        print("%s: relative top gap min %.2e, rows below 1e-6: %d of %d" % (name, g.min(), (g < 1e-6).sum(), len(g)))
        assert (g < 1e-6).sum() <= 0.05 * len(g)
        if name == "exact":
            qq = np.array([R.keypoints_to_quat(a, b, c) for a, b, c in zip(k1, k2, loc)])
            ang = R.angle(qq, q)
            print("exact: Kabsch vs pose: exact-in-fp32 rows %.2e rad, fp32-rounded rows %.2e rad (bound %.2e)" %
                  (ang[exact].max(), ang[~exact].max(), R.keypoint_input_bound(k1, k2, loc)))
            assert ang[exact].max() <= 1e-14 and ang[~exact].max() <= R.keypoint_input_bound(k1, k2, loc)
            k1e = np.array([R.encode_as_keypoints(qi, ci) for qi, ci in zip(q[exact], loc[exact].astype(np.float64))])
            assert np.array_equal(k1e[:, 0].astype(np.float32).astype(np.float64), k1e[:, 0])      # exact in fp32 indeed


# ------------------------------------------------------------------------------------------------ the gates reject mistakes
def _rejected_by(K, defect, families=None):
    """Which gates reject the emulation with `defect` on the cases of K."""
    z, fam, hq, A, M, _, _ = _emulated(K)
    rows = [i for i, f in enumerate(fam) if families is None or f in families]
    q, a = R.emulate_wavg(z[rows], hq, defect)
    out = set()
    if R.gate_scatter(a, A[rows], M[rows], K) > 1:
        out.add("scatter")
    if np.all(np.isfinite(a)) and R.gate_solver(q, a)[0] > 1:
        out.add("solver")
    if R.gate_decode(q, K, A[rows], M[rows])[0] > 1:
        out.add("decode")
    zp, ks = R.planted_cases(K)
    if R.gate_planted(R.emulate_wavg(zp, hq, defect)[0], hq[ks]) > 1:
        out.add("planted")
    return out


def test_gates_reject_summation_mistakes():
    got = {d: _rejected_by(1728, d) for d in ("tail_drop", "wave_drop", "map_fp16")}
    got["max256"] = _rejected_by(1728, "max256", ("range200",))
    print(got)
    assert {"scatter", "planted"} <= got["tail_drop"]            # a single bin of 1728 moves A by 1e-3 of its size; planted bin 1536 vanishes
    assert {"scatter", "planted"} <= got["wave_drop"]
    assert {"scatter", "planted"} <= got["map_fp16"]
    # a common factor cancels in A, so a short maximum shows only where it lets expf overflow: the planted bins past 255 (z - max = 200)
    assert "planted" in got["max256"]
    # the existing gate (|dot| > 1 - 1e-5) would pass the dropped tail bin and the fp16 map: that is the gap this file's gates close
    z, fam, hq, A, M, _, _ = _emulated(1728)
    v = R.top_vector(A)[0]
    for d in ("tail_drop", "map_fp16"):
        q, _ = R.emulate_wavg(z, hq, d)
        keep = [i for i, f in enumerate(fam) if f.startswith("peak")]
        dots = np.abs(np.sum(q[keep].astype(np.float64) * v[keep], axis=1))
        print(d, "old gate: 1 - |dot| =", 1 - dots)
        assert np.all(dots > 1 - 1e-5)


def test_gates_reject_solver_mistakes():
    rej_sign = set().union(*(_rejected_by(K, "no_sign") for K in (512, 1728)))
    print("no_sign:", rej_sign)
    assert "solver" in rej_sign
    rej_sweep = set().union(*(_rejected_by(K, "one_sweep", ("equal", "normal")) for K in (512, 1728, 13824)))
    print("one_sweep on the flat cases:", rej_sweep)
    assert "solver" in rej_sweep                                  # the Rayleigh quotient falls short of lambda1 by more than 1e-12 spread


def test_gates_reject_conversion_mistakes():
    e = R.euler_cases().astype(np.float64)
    Rs = [R.euler_to_so3(*x) for x in e]
    ref = np.array([R.so3_to_quat(Rm)[0] for Rm in Rs])
    br = np.array([R.so3_to_quat(Rm)[1] for Rm in Rs])
    # R00 > R11 replaced by >=: an EQUIVALENT variant -- at R00 == R11 both neighbouring branches are valid formulas of the same quaternion
    # (each branch divides by Z = 2 sqrt(1 + 2 R_kk - tr), nonzero on both sides of the tie), and on the 180-degree-about-z row
    # (diag(-1, -1, 1)) the second comparison R00 > R22 still fails, so the variant takes the same branch.  No gate can (or should) reject
    # it; asserted so that the claim is checked rather than believed.
    Rz = np.diag([-1.0, -1.0, 1.0])
    assert R.so3_to_quat(Rz, "ge")[1] == R.so3_to_quat(Rz)[1] == 3
    ge = np.array([R.so3_to_quat(Rm, "ge")[0] for Rm in Rs])
    assert R.gate_quat(ge, ref, 1e-12) <= 1 and R.gate_rotation(ge, Rs, 1e-12) <= 1
    # a branch mistake that IS one: the last branch's w with swapped operands -- seen only because that branch is reached
    w4 = np.array([R.so3_to_quat(Rm, "w4")[0] for Rm in Rs])
    assert R.gate_rotation(w4[br == 3], [Rs[i] for i in np.where(br == 3)[0]], 1e-12) > 1
    assert R.gate_rotation(w4[br != 3], [Rs[i] for i in np.where(br != 3)[0]], 1e-12) <= 1
    # the reflection left uncorrected in the keypoint solve
    cases, q, exact = R.keypoint_cases()
    k1, k2, loc = cases["exact"]
    good = np.array([R.keypoints_to_quat(a, b, c) for a, b, c in zip(k1, k2, loc)])
    bad = np.array([R.keypoints_to_quat(a, b, c, correct_reflection=False) for a, b, c in zip(k1, k2, loc)])
    with np.errstate(invalid="ignore"):
        wrong = ~(R.angle(bad, good) <= 1e-10)
    print("uncorrected reflection: %d of %d rows rejected" % (wrong.sum(), len(wrong)))
    assert wrong.sum() >= 8
