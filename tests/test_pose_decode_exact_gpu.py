"""Float64 probes of the pose decode on the device: urso_quat_wavg_decode (scatter, solver, launch), and the conversions and reductions of
urso_pose_eval / urso_pose_decode, against tests/poseref.py (proven on the CPU in tests/test_poseref_cpu.py, which also shows that these
gates reject a dropped tail bin, a dropped wave partial, an fp16 map, a short maximum, a missing sign rule and a solver stopped early).

Gates (eps = 2^-24; derivations in poseref's gate functions and DESIGN.md section 9):
  a  scatter       |a_d - A| <= (ceil(K/256) + 24) eps (M + |A|) + 1e-45 element by element; a_d symmetric; trace within 4 T of 1   derived
  b  planted bins  q = sign-normalised map row within 2^-23; two antipodal bins: +-normalise(h1 - h2) within 2^-22                 derived
  c  solver alone  on the kernel's own a_d: ||q - v|| <= 2^-23 + 1e-14 / gap, unit norm, Rayleigh quotient, sign rule               derived;
                   rows with gap < 1e-6 skip the vector comparison: only the "equal" family may (seed-dependent cap)
  d  end to end    angle(q, v64) <= 2 asin(|T|_F / (gap - |T|_F)) + 2^-21 (Davis-Kahan on the tolerance of a)                       derived;
                   rows with gap <= 4 |T|_F excluded: only "equal" (and "peak3" at K = 262,144) may be (seed-dependent cap)
  e  launch        B rows together = each alone, a_d optional, NaN / -inf stay in their row, bad arguments do not launch
  f  conversions   Euler: |R(q) - R_ref| <= 1e-12 and q = +-q_ref off the branch ties; angle-axis: |q - q_ref| <= 1e-14               derived
  g  keypoints     Horn on the device vs Kabsch / SVD in float64: 1e-9 / g; at most 5 % of rows under g < 1e-6 (seed-dependent cap)
  h  location and encoded targets: 1e-12 relative; ORI_ENC_ERR 1e-9 degree                                                          derived
These supersede the soft head's older gates in test_kernels_gpu.py / test_evaluate_gpu.py (tightened to 1 - 1e-9 on the golden sizes).

With URSO_POSE_DECODE_REPORT=<path> the largest observed / bound ratios per test and K are written there next to the CPU emulation's
(profiles/pose_decode_exact.txt is such a run)."""
import os

import numpy as np
import pytest
import torch

import poseref as R

pytestmark = pytest.mark.gpu
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("URSO_POSE_DECODE_REPORT")
    for line in REPORT:
        print(line)
    if path:
        with open(path, "w") as f:
            f.write("# tests/test_pose_decode_exact_gpu.py: largest observed / bound per test and K (<= 1 passes); emu = the fp32 emulation on the CPU\n")
            f.write("\n".join(REPORT) + "\n")


def _dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()


def _wavg(z, hq, want_a=True):
    """urso_quat_wavg_decode -> (q fp32 [B,4], a fp32 [B,16] or None) as NumPy."""
    from ursonet_amd import hip
    z, hq = (t if torch.is_tensor(t) else _dev(t, np.float32) for t in (z, hq))
    B, K = z.shape
    q = torch.full((B, 4), -7.0, dtype=torch.float32, device="cuda")
    a = torch.full((B, 16), -7.0, dtype=torch.float32, device="cuda") if want_a else None
    hip.quat_wavg_decode(B, K, z, hq, q, a)
    torch.cuda.synchronize()
    return q.cpu().numpy(), (a.cpu().numpy() if want_a else None)


RUNS = {}


def _run(K):
    """The cases of K decoded once: (z, families, map, A, M, q, a)."""
    if K not in RUNS:
        z, fam = R.logit_cases(K, big=K == R.K_BIG)
        hq = R.bin_map(K)
        A, M = R.scatter(z, hq)
        q, a = _wavg(z, hq)
        RUNS[K] = (z, fam, hq, A, M, q, a)
    return RUNS[K]


EMUS = {}


def _emu(K):
    """The CPU emulation of the same cases, once: (q, a)."""
    if K not in EMUS:
        z, _, hq = _run(K)[:3]
        EMUS[K] = R.emulate_wavg(z, hq)
    return EMUS[K]


ALL_K = R.KS


# ------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("K", ALL_K)
def test_scatter_elementwise(K):
    z, fam, hq, A, M, q, a = _run(K)
    assert len(fam) == (3 if K == R.K_BIG else 11)
    r = R.gate_scatter(a, A, M, K)
    emu = R.gate_scatter(_emu(K)[1], A, M, K)
    per = {f: R.gate_scatter(a[[i for i, g in enumerate(fam) if g == f]], A[[i for i, g in enumerate(fam) if g == f]],
                             M[[i for i, g in enumerate(fam) if g == f]], K) for f in sorted(set(fam))}
    REPORT.append("a scatter   K=%-6d gpu %.3f  emu %.3f  per family %s" % (K, r, emu, " ".join("%s %.3f" % kv for kv in per.items())))
    print(REPORT[-1])
    assert r <= 1


# ------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("K", ALL_K)
def test_planted_bins(K):
    hq = R.bin_map(K)
    zp, ks = R.planted_cases(K)
    assert ks == R.planted_bins(K) and (K < 512 or len(ks) >= 6) and (K % 256 == 0 or K < 256 or K - K % 256 in ks)
    qp, ap = _wavg(zp, hq)                                                # every planted bin of K in ONE launch
    r1 = R.gate_planted(qp, hq[ks])
    za, pairs = R.antipodal_cases(K)
    r2 = 0.0
    if pairs:
        h = hq.astype(np.float64)
        ref = np.array([h[i] - h[j] for i, j in pairs])
        r2 = R.gate_planted(_wavg(za, hq)[0], ref / np.linalg.norm(ref, axis=1, keepdims=True), tol=2.0 ** -22)
    e1 = R.gate_planted(R.emulate_wavg(zp, hq)[0], hq[ks])
    e2 = R.gate_planted(R.emulate_wavg(za, hq)[0], ref / np.linalg.norm(ref, axis=1, keepdims=True), tol=2.0 ** -22) if pairs else 0.0
    REPORT.append("b planted   K=%-6d gpu single %.3f  emu %.3f  antipodal %.3f  emu %.3f (%d pairs)" % (K, r1, e1, r2, e2, len(pairs)))
    print(REPORT[-1])
    assert r1 <= 1 and r2 <= 1
    # the scatter of a planted bin is the rounded outer product of its map row
    hk = hq[ks].astype(np.float64)
    assert np.abs(ap.reshape(-1, 4, 4) - hk[:, :, None] * hk[:, None, :]).max() <= 2 * R.EPS


# ------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("K", ALL_K)
def test_solver_alone(K):
    z, fam, hq, A, M, q, a = _run(K)
    r, low = R.gate_solver(q, a)
    zq, za = _emu(K)
    REPORT.append("c solver    K=%-6d gpu %.3f  emu %.3f  rows below gap 1e-6: %s" % (K, r, R.gate_solver(zq, za)[0], [fam[i] for i in np.where(low)[0]]))
    print(REPORT[-1])
    assert r <= 1
    assert {fam[i] for i in np.where(low)[0]} <= {"equal"}


# ------------------------------------------------------------------------------------------------ d
@pytest.mark.parametrize("K", ALL_K)
def test_decode_end_to_end(K):
    z, fam, hq, A, M, q, a = _run(K)
    r, excl = R.gate_decode(q, K, A, M)
    emu = R.gate_decode(_emu(K)[0], K, A, M)[0]
    v = R.top_vector(A[~excl])[0]
    REPORT.append("d decode    K=%-6d gpu %.3f  emu %.3f  largest angle %.2e rad  excluded: %s" %
                  (K, r, emu, R.angle(q[~excl], v).max() if (~excl).any() else 0.0, [fam[i] for i in np.where(excl)[0]]))
    print(REPORT[-1])
    assert r <= 1
    assert {fam[i] for i in np.where(excl)[0]} <= ({"equal", "peak3"} if K == R.K_BIG else {"equal"})


def test_k262144_every_gate():
    """The released weights' 64^3 bins, B = 3 (peak3, peak12, equal): each thread adds 1024 terms in fp32.  Gates a, b, c, d in one test."""
    for check in (test_scatter_elementwise, test_planted_bins, test_solver_alone, test_decode_end_to_end):
        check(R.K_BIG)


# ------------------------------------------------------------------------------------------------ e
def _rows37(K):
    z, _ = R.logit_cases(K)
    z2, _ = R.logit_cases(K, seed=1)
    z3, _ = R.logit_cases(K, seed=2)
    z4, _ = R.logit_cases(K, seed=3)
    return np.concatenate([z, z2, z3, z4])[:37]


def test_rows_together_equal_rows_alone_and_scatter_is_optional():
    K = 1728
    z, hq = _dev(_rows37(K)), _dev(R.bin_map(K))
    assert z.shape[0] == 37
    q, a = _wavg(z, hq)
    q_no_a, _ = _wavg(z, hq, want_a=False)
    assert np.array_equal(q.view(np.uint32), q_no_a.view(np.uint32))
    for b in range(37):
        qb, ab = _wavg(z[b:b + 1], hq)
        assert np.array_equal(qb.view(np.uint32), q[b:b + 1].view(np.uint32)) and np.array_equal(ab.view(np.uint32), a[b:b + 1].view(np.uint32)), b


def test_nan_and_all_neginf_rows_stay_in_their_row():
    K = 1728
    z = _rows37(K)[:12]
    hq = R.bin_map(K)
    q0, a0 = _wavg(z, hq)
    assert np.all(np.isfinite(q0)) and np.all(np.isfinite(a0))
    z1 = z.copy()
    z1[3, 1700] = np.nan                                                  # in the ragged tail
    z1[7, :] = -np.inf
    z1[9, 0] = np.nan
    q1, a1 = _wavg(z1, hq)
    bad = [3, 7, 9]
    good = [b for b in range(12) if b not in bad]
    assert np.all(np.isnan(q1[bad])) and np.all(np.isnan(a1[bad]))
    assert np.array_equal(q1[good].view(np.uint32), q0[good].view(np.uint32)) and np.array_equal(a1[good].view(np.uint32), a0[good].view(np.uint32))


def test_bad_arguments_do_not_launch():
    from ursonet_amd import hip
    K, B = 512, 4
    z = _dev(R.logit_cases(K)[0][:B])
    hq = _dev(R.bin_map(K))
    off = torch.zeros(K * 4 + 4, dtype=torch.float32, device="cuda")
    assert off.data_ptr() % 16 == 0
    hq_off = off[1:1 + K * 4]                                             # 4 bytes past a 16-byte boundary
    q = torch.full((B, 4), -7.0, dtype=torch.float32, device="cuda")
    a = torch.full((B, 16), -7.0, dtype=torch.float32, device="cuda")
    for args, what in (((B, 0, z, hq, q, a), "bad argument"), ((B, -5, z, hq, q, a), "bad argument"), ((0, K, z, hq, q, a), "bad argument"),
                       ((-1, K, z, hq, q, a), "bad argument"), ((B, K, None, hq, q, a), "bad argument"), ((B, K, z, None, q, a), "bad argument"),
                       ((B, K, z, hq_off, q, a), "16-byte aligned")):
        with pytest.raises(hip.UrsoHipError, match=what):
            hip.quat_wavg_decode(*args)
    with pytest.raises(hip.UrsoHipError, match="bad argument"):
        hip.quat_wavg_decode(B, K, z, hq, None, a)
    torch.cuda.synchronize()
    assert bool((q == -7.0).all()) and bool((a == -7.0).all())


# ------------------------------------------------------------------------------------------------ f, g: urso_pose_decode, regressed location
def _pose_decode(ori_mode, ori, loc=None, ori2=None):
    """urso_pose_decode with a regressed location on fp32 rows -> the Q_EST columns [N,4] float64 (and the whole table)."""
    from ursonet_amd import hip
    ori = np.asarray(ori, dtype=np.float32)
    N = len(ori)
    loc = np.tile(np.float32([0.5, -0.25, 12.0]), (N, 1)) if loc is None else np.asarray(loc, dtype=np.float32)
    t = torch.full((N, hip.DEC_COLS), -7.0, dtype=torch.float64, device="cuda")
    hip.pose_decode(N, N, 0, hip.EVAL_LOC_REGRESS, ori_mode, _dev(loc), _dev(ori), t, ori2=None if ori2 is None else _dev(ori2, np.float32))
    torch.cuda.synchronize()
    t = t.cpu().numpy()
    assert np.array_equal(t[:, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3], loc.astype(np.float64))
    return t[:, hip.DEC_Q_EST:hip.DEC_Q_EST + 4], t


def test_euler_to_quaternion_every_branch():
    from ursonet_amd import hip
    e = R.euler_cases()
    q, _ = _pose_decode(hip.EVAL_ORI_EULER, e)
    Rs = [R.euler_to_so3(*x.astype(np.float64)) for x in e]
    ref = [R.so3_to_quat(Rm) for Rm in Rs]
    qr, br = np.array([r[0] for r in ref]), np.array([r[1] for r in ref])
    off = np.array([R.so3_branch_margin(Rm) >= 1e-12 for Rm in Rs])
    assert np.all(np.bincount(br, minlength=4) >= 8) and np.all(np.bincount(br[off], minlength=4) >= 8)
    r_mat, r_q = R.gate_rotation(q, Rs, 1e-12), R.gate_quat(q[off], qr[off], 1e-12)
    REPORT.append("f euler     rows %d (per branch %s, %d within 1e-12 of a tie): matrix %.3f  quaternion off ties %.3f" %
                  (len(e), np.bincount(br, minlength=4), (~off).sum(), r_mat, r_q))
    print(REPORT[-1])
    assert r_mat <= 1 and r_q <= 1
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-12


def test_angle_axis_small_and_large_angles():
    from ursonet_amd import hip
    v = R.angle_axis_cases()
    assert len(v) == 40
    q, _ = _pose_decode(hip.EVAL_ORI_ANGLE_AXIS, v)
    ref = np.array([R.angle_axis_to_quat(x) for x in v])
    th = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.sum((th > 0) & (th < 1e-6)) >= 8 and np.sum(th > 6) >= 12   # both sides of the reference's cut, and past a full turn
    assert np.all(q[th < 1e-6, :3] == 0)
    r = float(np.abs(q - ref).max() / 1e-14)
    REPORT.append("f angleaxis rows %d: %.3f" % (len(v), r))
    print(REPORT[-1])
    assert r <= 1


def test_keypoints_against_kabsch():
    from ursonet_amd import hip
    cases, pose, exact = R.keypoint_cases()
    for name, (k1, k2, loc) in cases.items():
        q, _ = _pose_decode(hip.EVAL_ORI_KEYPOINTS, k1, loc=loc, ori2=k2)
        ref = np.array([R.keypoints_to_quat(a, b, c) for a, b, c in zip(k1, k2, loc)])
        g = np.array([R.horn_gap(a, b, c) for a, b, c in zip(k1, k2, loc)])
        keep = g >= 1e-6
        assert (~keep).sum() <= 0.05 * len(g)
        assert np.all(np.isfinite(q)) and np.abs(np.linalg.norm(q, axis=1) - 1).max() <= 1e-12
        dR = np.array([np.abs(R.quat_to_so3(a) - R.quat_to_so3(b)).max() for a, b in zip(q, ref)])
        r = float((dR[keep] * g[keep] / 1e-9).max())
        line = "g keypoints %-10s rows %d: |R(q) - R(q_ref)| g / 1e-9 = %.2e" % (name, keep.sum(), r)
        assert r <= 1, line
        if not name.startswith("noise"):
            # exact encodings and their rescalings: the fit of the same fp32 values within 1e-10; the pose itself within 1e-10 where the
            # keypoints are exact in fp32, elsewhere within the rounding of the fp32 inputs
            a_ref, a_pose = R.angle(q, ref), R.angle(q, pose)
            bound = R.keypoint_input_bound(k1, k2, loc) if name == "exact" else 4 * np.sqrt(3.0) * 2.0 ** -23
            line += "  angle to the fit %.2e, to the pose: exact rows %.2e, rounded rows %.2e (bound %.2e)" % (
                a_ref.max(), a_pose[exact].max(), a_pose[~exact].max(), bound)
            assert a_ref.max() <= 1e-10 and a_pose[exact].max() <= 1e-10 and a_pose[~exact].max() <= bound, line
        REPORT.append(line)
        print(line)


def test_degenerate_keypoints_are_finite_and_repeatable():
    from ursonet_amd import hip
    loc = np.float32([[0.5, -0.25, 12.0]] * 6)
    d = np.float32([0.6, 0.0, 0.8])
    k1 = loc + np.float32([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [0.6, 0, 0.8], [1e-30, 0, 0]])
    k2 = loc + np.float32([[0, 0, 0], [2, 0, 0], [0, 1, 0], [1, 0, 0], [-1.2, 0, -1.6], [0, 1e-30, 0]])
    assert np.allclose((k2 - loc)[4], -2 * d)                             # rows: coincident, collinear, k1 = loc, k1 = k2, collinear opposite, tiny
    q1, t1 = _pose_decode(hip.EVAL_ORI_KEYPOINTS, k1, loc=loc, ori2=k2)
    q2, t2 = _pose_decode(hip.EVAL_ORI_KEYPOINTS, k1, loc=loc, ori2=k2)
    assert np.all(np.isfinite(t1[:, :7])) and np.abs(np.linalg.norm(q1, axis=1) - 1).max() <= 1e-12
    assert np.array_equal(t1.view(np.uint64), t2.view(np.uint64))


# ------------------------------------------------------------------------------------------------ h
LOC_MAX, LOC_MIN = (0.45, 0.35, 40.0), (-0.45, -0.35, 3.0)


def _loc_logits(K, seed):
    rng = np.random.default_rng(6000 + seed + K)
    rows = [rng.standard_normal(K), 4 * rng.standard_normal(K), rng.uniform(-100, 100, K), rng.uniform(-100, 100, K)]
    for _ in range(2):
        r = rng.standard_normal(K)
        r[rng.random(K) < 0.3] = -np.inf
        r[rng.integers(K)] = 0.25
        rows.append(r)
    return np.stack(rows).astype(np.float32), ["normal", "normal", "range200", "range200", "neginf", "neginf"]


def _padded(x, fill=1e30, extra=5):
    """Device tensor whose rows are `extra` floats further apart than they are long, the padding filled."""
    buf = torch.full((x.shape[0], x.shape[1] + extra), fill, dtype=torch.float32, device="cuda")
    buf[:, :x.shape[1]] = torch.as_tensor(x)
    return buf[:, :x.shape[1]]


def _rel(a, b):
    return float((np.abs(a - b) / np.abs(b)).max())


@pytest.mark.parametrize("m", [1, 4, 7, 10, 24])
def test_classified_location_and_encoded_targets(m):
    from ursonet_amd import hip
    from ursonet_amd.pose import OrientationCodec, location_map
    K = m ** 3
    lm = location_map(m, LOC_MAX, LOC_MIN)
    z, fam = _loc_logits(K, 0)
    B = len(z)
    rng = np.random.default_rng(7000 + m)
    # orientation side: soft head over n^3 bins, encoded targets of random poses, q_gt 10..90 degrees away from them
    n = max(m, 4)
    codec = OrientationCodec(n, 6.0)
    hq, Ko = codec.H_quat, n ** 3
    zo, _ = _loc_logits(Ko, 1)
    pose = R.random_quats(rng, B)
    enc_ori = codec.encode(pose)
    assert enc_ori.dtype == np.float32 and np.all(np.isfinite(enc_ori))
    perp = rng.standard_normal((B, 4))
    perp -= np.sum(perp * pose, axis=1, keepdims=True) * pose
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    phi = np.radians(rng.uniform(10, 90, B))[:, None]
    q_gt = np.cos(phi / 2) * pose + np.sin(phi / 2) * perp
    enc_loc = np.exp(3 * rng.standard_normal((B, K)))
    enc_loc = (enc_loc / enc_loc.sum(axis=1, keepdims=True)).astype(np.float32)
    loc_gt = rng.uniform(-1, 1, (B, 3)) * [3, 3, 15] + [0, 0, 20]

    zd, zod, hqd, lmd = _padded(z), _padded(zo), _dev(hq), _dev(lm)
    q_soft = torch.empty(B, 4, dtype=torch.float32, device="cuda")
    hip.quat_wavg_decode(B, Ko, _dev(zo), hqd, q_soft)
    td = torch.full((B, hip.DEC_COLS), -7.0, dtype=torch.float64, device="cuda")
    hip.pose_decode(B, B, 0, hip.EVAL_LOC_CLASS, hip.EVAL_ORI_SOFT, zd, q_soft, td, loc_map=lmd, ori_logits=zod, ori_map_rows=Ko)
    te = torch.full((B, hip.EVAL_COLS), -7.0, dtype=torch.float64, device="cuda")
    hip.pose_eval(B, B, 0, hip.EVAL_LOC_CLASS, hip.EVAL_ORI_SOFT, zd, q_soft, _dev(loc_gt), _dev(q_gt), te, loc_map=lmd, ori_map=hqd,
                  enc_loc=_dev(enc_loc), enc_ori=_dev(enc_ori))
    torch.cuda.synchronize()
    td, te = td.cpu().numpy(), te.cpu().numpy()

    est, pk = R.loc_softmax(z, lm)
    r_est = float(np.abs(td[:, hip.DEC_LOC_EST:hip.DEC_LOC_EST + 3] - est).max() / (1e-12 * np.abs(lm).max()))
    r_lpk = _rel(td[:, hip.DEC_LOC_PEAK], pk) / 1e-12
    r_opk = _rel(td[:, hip.DEC_ORI_PEAK], R.peak(zo)) / 1e-12
    enc_ref = np.linalg.norm(R.first_moment(enc_loc, lm) - loc_gt, axis=1)
    r_lenc = _rel(te[:, hip.EVAL_LOC_ENC_ERR], enc_ref) / 1e-12
    v, gap, _ = R.top_vector(R.pmf_scatter(enc_ori, hq))
    ori_ref = np.degrees(2 * np.arccos(np.minimum(1.0, np.abs(np.sum(v * q_gt, axis=1)))))
    assert np.all(ori_ref >= 5.0)
    r_oenc = float(np.abs(te[:, hip.EVAL_ORI_ENC_ERR] - ori_ref).max() / 1e-9)
    REPORT.append("h location  m=%-2d K=%-5d loc_est %.3f  LOC_PEAK %.3f  ORI_PEAK %.3f  LOC_ENC_ERR %.3f  ORI_ENC_ERR (n=%d) %.2e" %
                  (m, K, r_est, r_lpk, r_opk, r_lenc, n, r_oenc))
    print(REPORT[-1])
    assert max(r_est, r_lpk, r_opk, r_lenc, r_oenc) <= 1
    # both entry points write the same LOC_EST and Q_EST bits, and Q_EST is the soft decode's q
    assert np.array_equal(td[:, :7].view(np.uint64), te[:, :7].view(np.uint64))
    assert np.array_equal(td[:, hip.DEC_Q_EST:hip.DEC_Q_EST + 4], q_soft.cpu().numpy().astype(np.float64))
