"""Temperature scaling on the GPU: urso_temp_stats / urso_temp_reduce / urso_temp_scale against their float64 statement
(ursonet_amd.calibrate.stats64 / reduce64 / scale32; cases and bounds: tests/tempref.py), their determinism, fit_temperature against
fit64, and calibrate() / predict / evaluate with calibration=... end to end on the small model and dataset of tests/test_ensemble_gpu.py."""
import numpy as np
import pytest
import torch

import poseref as P
import tempref as R
from ursonet_amd import calibrate as Cal
from util import make_config

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32).copy()


class _Case(object):
    """The device buffers of one urso_temp_stats case, NaN wherever the kernel must neither read nor write: logits and targets sit
    `misalign` floats (the targets one more) behind a 16-byte boundary in rows ld apart; the table has rows in front of row0 and behind
    row0 + n, and its columns behind 2 + 3 J are not written either."""

    def __init__(self, K, B, n, row0, ld, misalign=1):
        rows = row0 + B + 1
        self.K, self.B, self.n, self.row0, self.ld, self.rows, self.mis = K, B, n, row0, ld, rows, misalign
        self.zstore = torch.full((B * ld + 8,), NAN, dtype=torch.float32, device="cuda")
        self.ystore = torch.full((B * ld + 8,), NAN, dtype=torch.float32, device="cuda")
        ymis = misalign + 1 if misalign else 0
        self.ymis = ymis
        self.logits = self.zstore[misalign:misalign + B * ld].view(B, ld)[:, :K]
        self.target = self.ystore[ymis:ymis + B * ld].view(B, ld)[:, :K]
        assert self.logits.data_ptr() % 16 == 4 * (misalign % 4) and self.target.data_ptr() % 16 == 4 * (ymis % 4)
        self.out = torch.full((rows, Cal.COLS), NAN, dtype=torch.float64, device="cuda")

    def run(self, z, y, betas):
        """-> the table rows of the n valid batch rows [n, 2 + 3 J], after checking every untouched element."""
        from ursonet_amd import hip
        J = len(betas)
        self.logits[:self.n] = _dev(z)
        self.target[:self.n] = _dev(y)
        hip.temp_stats(self.B, self.n, self.row0, betas, self.logits, self.target, self.out)
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        keep = np.ones(self.rows, dtype=bool)
        keep[self.row0:self.row0 + self.n] = False
        assert np.all(np.isnan(out[keep])), "a row outside [row0, row0 + n) was written"
        assert np.all(np.isnan(out[:, 2 + 3 * J:])), "a column behind 2 + 3 J was written"
        for store, mis, src in ((self.zstore, self.mis, z), (self.ystore, self.ymis, y)):
            pad = store.cpu().numpy().copy()
            body = pad[mis:mis + self.B * self.ld].reshape(self.B, self.ld)[:self.n, :self.K]
            assert np.array_equal(body.view(np.int32), np.asarray(src, dtype=np.float32).view(np.int32)), "an input was written"
            body[...] = NAN
            assert np.all(np.isnan(pad)), "the padding of an input was written"
        return self.out[self.row0:self.row0 + self.n, :2 + 3 * J]


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("K", R.KS + (R.BIG_K,))
def test_stats_against_the_float64_statement(K, scale):
    """urso_temp_stats on normal logits of the given scale at J = 1, 3, 8 temperatures (K = 32768: J = 8, packed), B = 3, n = 2, row0 = 5,
    ld = K + 3, logits one float and targets two floats off the 16-byte boundary, every buffer NaN around the valid elements; scale 1 has
    a -inf bin, scale 30 a NaN row (NaN in every column, the other row finite) and a zero target row.  Bounds of tests/tempref.py:
    SY, YZ within K 2^-52 of the sums of magnitudes, LSE and M1 within (K + 16) 2^-52 of their two parts, VAR within that times
    (Q / Z + (A / Z)^2)."""
    B, n, row0, ld = R.shape_of(K)
    z, y = R.logits_and_targets(K, scale)
    for J in (R.JS if K != R.BIG_K else (8,)):
        betas = R.betas_of(J)
        got = _Case(K, B, n, row0, ld, misalign=0 if K == R.BIG_K else 1).run(z, y, betas).cpu().numpy()
        fig = R.check_stats(got, z, y, betas)
        print("K=%d J=%d scale=%g observed / bound:" % (K, J, scale), {k: "%.3g" % v for k, v in fig.items()})
        if K > 1 and scale != 1.0:
            assert np.all(np.isnan(got[1])) and np.all(np.isfinite(got[0])) and got[0, Cal.SY] == 0 and got[0, Cal.YZ] == 0
        else:
            assert np.all(np.isfinite(got))
        for k, v in fig.items():
            assert v <= 1, (K, J, scale, k, fig)


@pytest.mark.parametrize("K", [63, 257, 4096])
def test_stats_are_a_function_of_the_row_alone(K):
    """Two launches give equal bits; the row at (B, n, row0) = (3, 2, 5) in padded, misaligned rows and the same row alone at
    (1, 1, 0), packed, aligned or two floats off, give equal bits -- the NaN row included; and a temperature's columns do not depend on
    which other temperatures share the launch."""
    z, y = R.logits_and_targets(K, 30.0)
    y[0] = R.logits_and_targets(K, 1.0)[1][0]                                  # (a target that is not zero)
    betas = R.betas_of(8)
    first = _bits(_Case(K, 3, 2, 5, K + 3).run(z, y, betas))
    again = _bits(_Case(K, 3, 2, 5, K + 3).run(z, y, betas))
    assert np.array_equal(first, again)
    for r in (0, 1):
        for mis in (0, 2):
            alone = _bits(_Case(K, 1, 1, 0, K, misalign=mis).run(z[r:r + 1], y[r:r + 1], betas))
            assert np.array_equal(first[r], alone[0]), (r, mis)
    for j in (0, 3, 7):
        single = _bits(_Case(K, 3, 2, 5, K + 3).run(z, y, [betas[j]]))
        assert np.array_equal(single[:, :2], first[:, :2]) and np.array_equal(single[:, 2:5], first[:, 2 + 3 * j:5 + 3 * j]), j


@pytest.mark.parametrize("N", [1, 1023, 1025, 3000])
def test_reduce_against_the_sum_of_its_own_rows(N):
    """urso_temp_reduce over a table urso_temp_stats wrote: the per-row terms are single IEEE operations in the header's order, which
    NumPy repeats exactly, so the totals differ from the float64 sum of those terms by the order of N - 1 additions alone -- within
    N 2^-52 of the sum of the terms' magnitudes (for CE and h, whose terms have one sign here, that is N 2^-52 relative).  Then three rows
    are made non-finite (a NaN, an inf, a NaN in one temperature's column only) and the count must say so per temperature."""
    from ursonet_amd import hip
    K, J = 16, 8
    betas = R.betas_of(J)
    rng = np.random.default_rng(N)
    z = rng.normal(size=(N, K)).astype(np.float32) * 2
    y = rng.uniform(0, 1, size=(N, K)).astype(np.float32)
    rows = torch.full((N + 2, Cal.COLS), NAN, dtype=torch.float64, device="cuda")
    hip.temp_stats(N, N, 0, betas, _dev(z), _dev(y), rows)
    totals = torch.full((Cal.MAX_J, Cal.TOTALS), NAN, dtype=torch.float64, device="cuda")
    for Jr in (8, 3):
        totals.fill_(NAN)
        hip.temp_reduce(N, betas[:Jr], rows, totals)
        got = totals.cpu().numpy()
        assert np.all(np.isnan(got[Jr:])) and np.all(got[:Jr, 3] == 0)
        ce, g, h, bad = Cal.row_terms(rows.cpu().numpy()[:N], betas[:Jr])
        assert not bad.any() and np.all(ce > 0) and np.all(h >= 0)
        for col, terms in enumerate((ce, g, h)):
            err = np.abs(got[:Jr, col] - terms.sum(axis=0)) / (N * R.EPS * np.abs(terms).sum(axis=0))
            print("N=%d J=%d column %d observed / bound %.3g" % (N, Jr, col, err.max()))
            assert np.all(err <= 1), (N, Jr, col, err)
        if N == 1:
            assert np.array_equal(got[:Jr, :3], np.stack([ce[0], g[0], h[0]], axis=1))
    again = totals.clone()
    hip.temp_reduce(N, betas[:3], rows, totals)
    assert np.array_equal(_bits(again[:3]), _bits(totals[:3]))
    if N >= 1023:
        rows[5, Cal.SY] = NAN
        rows[N - 1, Cal.YZ] = float("inf")
        rows[700, Cal.M1 + 3 * 2] = NAN
        hip.temp_reduce(N, betas, rows, totals)
        got = totals.cpu().numpy()
        assert list(got[:, 3]) == [2, 2, 3, 2, 2, 2, 2, 2] and not np.isfinite(got[:, :3]).any()


@pytest.mark.parametrize("K", [1, 3, 63, 64, 4097])
def test_scale_is_the_rounded_product_bit_for_bit(K):
    """urso_temp_scale against fl32(fp64(z) * beta): ragged K, rows off the 16-byte boundary on either side, NaN and +-inf passing through,
    beta = 1 the identity on the bits, nothing written behind K, past n or in the input."""
    from ursonet_amd import hip
    B, n, ld_in, ld_out = 3, 2, K + 3, K + 1
    rng = np.random.default_rng(K)
    z = (rng.normal(size=(n, K)) * 10).astype(np.float32)
    z[0, 0] = np.inf
    z[-1, K // 2] = -np.inf
    z[0, K - 1] = NAN
    if K > 3:
        z[1, 1], z[1, 2] = np.float32(1e-42), np.float32(-0.0)                 # a subnormal and a signed zero
    for beta in (1.0, 2.0, 0.1, 1.0 / 3, 64.0, 1.0 / 64, 1e-3):
        for mi, mo in ((0, 0), (1, 2), (3, 0)):
            src = torch.full((B * ld_in + 8,), NAN, dtype=torch.float32, device="cuda")
            dst = torch.full((B * ld_out + 8,), NAN, dtype=torch.float32, device="cuda")
            s, d = src[mi:mi + B * ld_in].view(B, ld_in)[:, :K], dst[mo:mo + B * ld_out].view(B, ld_out)[:, :K]
            s[:n] = _dev(z)
            before = _bits(src)
            hip.temp_scale(B, n, beta, s, d)
            torch.cuda.synchronize()
            assert np.array_equal(_bits(src), before), "the input was written"
            want = Cal.scale32(z, beta)
            got = dst.cpu().numpy().copy()
            body = got[mo:mo + B * ld_out].reshape(B, ld_out)[:n, :K]
            assert np.array_equal(body.view(np.int32), want.view(np.int32)), (K, beta, mi, mo)
            if beta == 1.0:
                assert np.array_equal(body.view(np.int32), z.view(np.int32))
            body[...] = NAN
            assert np.all(np.isnan(got)), "an element behind K or past n was written"
    x = _dev(z)
    hip.temp_scale(n, n, 0.1, x, x)                                           # in place
    assert np.array_equal(_bits(x), Cal.scale32(z, 0.1).view(np.int32))


@pytest.mark.parametrize("b0", R.PLANT_B0)
@pytest.mark.parametrize("K", R.PLANT_KS)
def test_fit_temperature_against_fit64(K, b0):
    """The search on the device against the reference root (fit64 at tol 1e-13), within tempref's bound TOL beta + delta_g / h, in at
    most 16 passes; the losses it reports are the reference's within the kernel bound."""
    z, y = R.planted(K, b0)
    ref, rinfo = Cal.fit64(z, y, tol=R.REF_TOL)
    beta, info = Cal.fit_temperature(_dev(z), _dev(y))
    bound = R.beta_bound(z, y, ref)
    print("K=%d b0=%g: device beta %.15g, reference %.15g, |difference| / bound %.3g, passes %d" % (K, b0, beta, ref, abs(beta - ref) / bound, info["passes"]))
    assert rinfo["converged"] and info["converged"] and not info["clamped"] and not info["flat"] and info["passes"] <= Cal.MAX_PASSES
    assert abs(beta - ref) <= bound
    host, hinfo = Cal.fit64(z, y)
    assert abs(info["nll_before"] - hinfo["nll_before"]) <= 2 * R.tol(K) * hinfo["nll_before"]
    assert abs(info["nll_after"] - hinfo["nll_after"]) <= 2 * R.tol(K) * hinfo["nll_after"] + abs(hinfo["g"]) * abs(beta - host) / len(z) + 1e-18


def test_fit_temperature_ends():
    """Clamped at either bound, flat, and the refusal of rows that are not finite, on the device as in fit64; more rows than one stats
    launch takes (STATS_CHUNK) give the fit of the same rows in one launch."""
    z, y = R.planted(63, 1.0)
    sharp = np.zeros_like(y)
    sharp[np.arange(len(z)), z.argmax(axis=1)] = 1
    for target, end in ((sharp, Cal.BETA_MAX), (np.full_like(y, 1.0 / 63), Cal.BETA_MIN)):
        beta, info = Cal.fit_temperature(_dev(z), _dev(target))
        assert beta == end and info["clamped"] and info["passes"] == Cal.fit64(z, target)[1]["passes"]
    beta, info = Cal.fit_temperature(_dev(np.full_like(z, 0.75)), _dev(y))
    assert beta == 1.0 and info["flat"] and info["passes"] == 1
    bad = z.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match=r"1 of %d rows are not finite" % len(z)):
        Cal.fit_temperature(_dev(bad), _dev(y))
    whole = Cal.fit_temperature(_dev(z), _dev(y))
    old = Cal.STATS_CHUNK
    Cal.STATS_CHUNK = 7
    try:
        parts = Cal.fit_temperature(_dev(z), _dev(y))
    finally:
        Cal.STATS_CHUNK = old
    assert parts[0] == whole[0] and parts[1] == whole[1]


# ------------------------------------------------------------------ end to end
_CACHE = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("calibrate")


def _setup(workdir, regress_loc):
    """(cfg, model, dataset): an inference ResNet-18 at 128 x 192 with the soft orientation head (8^3 bins), engine batch 3, 7 images
    (two batches and a tail of one) -- the model of tests/test_ensemble_gpu.py."""
    if regress_loc in _CACHE:
        return _CACHE[regress_loc]
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    cfg = make_config("resnet18", 128, 192, batch=3, regress_ori=False, regress_loc=regress_loc, ori_bins=8, loc_bins=4, dtype="float32")
    cfg.NAME = "syn"
    d = workdir / ("m%d" % regress_loc)
    d.mkdir()
    tr = net.UrsoNet(mode="training", config=cfg, model_dir=str(d))
    path = str(d / "weights_a_0001.npz")
    tr.save_weights(path)
    del tr
    model = net.UrsoNet(mode="inference", config=cfg, model_dir=str(d))
    model.load_weights(path, path, by_name=True)
    ds = SyntheticPoses(7, 128, 192, cfg, seed=3)
    ds._image_ids = np.array([3, 1, 4, 0, 6, 2, 5])
    _CACHE[regress_loc] = (cfg, model, ds)
    return _CACHE[regress_loc]


def _state_bits(model):
    eng = model._engine
    return eng.flat_w.detach().cpu().numpy().view(np.int32).copy(), eng.flat_stats.detach().cpu().numpy().view(np.int32).copy()


def _engine_logits(model, ds, ids=None):
    """The engine's own outputs over the dataset at predict()'s batch composition, and the output buffers' bits after the last batch:
    (loc [N, n_loc], ori [N, n_ori])."""
    from ursonet_amd.feeder import eval_batch_plan
    eng = model._engine
    locs, oris = [], []
    for _row0, n, slots in eval_batch_plan(ds.image_ids if ids is None else ids, eng.B):
        model.detect([ds.load_image(i) for i in slots])
        loc, ori = eng.outputs()
        locs.append(loc[:n].cpu().numpy().copy()); oris.append(ori[:n].cpu().numpy().copy())
    return np.concatenate(locs), np.concatenate(oris)


def _output_bits(model):
    loc, ori = model._engine.outputs()
    return _bits(loc.contiguous()), _bits(ori.contiguous())


def _same(a, b, keys):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True), k


PKEYS = ("image_ids", "loc_est", "q_est", "loc_peak", "ori_peak", "ori_lambda", "loc_spread", "ori_spread", "view_lambda", "n_views")


@pytest.mark.parametrize("regress_loc", [True, False])
def test_calibrate_is_fit64_on_the_engines_logits(workdir, regress_loc):
    """calibrate() against fit64 on logits read from the engine and the dataset's stored encoded targets, within tempref's bound; the
    weights, the BN statistics and a Calibration file come through unchanged; nr_images fits the first images only."""
    cfg, model, ds = _setup(workdir, regress_loc)
    before = _state_bits(model)
    cal = Cal.calibrate(model, ds)
    after = _state_bits(model)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    loc_z, ori_z = _engine_logits(model, ds)
    ori_y = np.stack([np.asarray(ds.load_orientation_encoded(i), dtype=np.float32) for i in ds.image_ids])
    heads = [("ori", ori_z, ori_y)]
    if not regress_loc:
        heads.append(("loc", loc_z, np.stack([np.asarray(ds.load_location_encoded(i), dtype=np.float32) for i in ds.image_ids])))
    assert cal.n_images == 7 and cal.k_ori == 512 and cal.k_loc == (None if regress_loc else 64) and (cal.loc_beta is None) == regress_loc
    for name, z, y in heads:
        ref, rinfo = Cal.fit64(z, y, tol=R.REF_TOL)
        host, hinfo = Cal.fit64(z, y)
        beta, fit = getattr(cal, name + "_beta"), getattr(cal, name + "_fit")
        print(name, "beta", beta, "reference", ref, "clamped", fit["clamped"], "passes", fit["passes"], "nll", fit["nll_before"], "->", fit["nll_after"])
        assert fit["clamped"] == hinfo["clamped"] and fit["flat"] is False and fit["converged"] and fit["passes"] <= Cal.MAX_PASSES
        assert beta == ref if fit["clamped"] else abs(beta - ref) <= R.beta_bound(z, y, ref)
        assert fit["nll_after"] <= fit["nll_before"] * (1 + R.tol(z.shape[1]))
        assert abs(fit["nll_before"] - hinfo["nll_before"]) <= 2 * R.tol(z.shape[1]) * abs(hinfo["nll_before"])
    again = Cal.Calibration.load(cal.save(str(workdir / ("cal%d.json" % regress_loc))))
    assert again == cal and again.ori_beta.hex() == cal.ori_beta.hex()
    few = Cal.calibrate(model, ds, nr_images=4)
    ref4 = Cal.fit64(ori_z[:4], ori_y[:4], tol=R.REF_TOL)[0]
    assert few.n_images == 4 and (few.ori_beta == ref4 if few.ori_clamped else abs(few.ori_beta - ref4) <= R.beta_bound(ori_z[:4], ori_y[:4], ref4))
    with pytest.raises(ValueError, match=r"calibrate: the logits and targets of 7 images \(512 orientation and %d location bins in fp32\) need 0\.000 GiB"
                                         % (0 if regress_loc else 64)):
        Cal.calibrate(model, ds, max_gb=1e-9)


def test_predict_and_evaluate_apply_the_calibration(workdir, capsys):
    """calibration=None and beta = 1 are the plain call bit for bit; beta = 2 gives the peak and the decode of softmax64(2 z), under the
    bounds the plain decode is tested with (tests/test_predict_gpu.py, tests/poseref.py), and another q_est than the plain call;
    evaluate scores the q_est that predict returns and prints the temperatures as a fifth line; views and multimodal go through the
    same scaled logits; the engine's outputs, weights and statistics are unchanged by every call."""
    from ursonet_amd import evaluate as ev, predict as pr
    cfg, model, ds = _setup(workdir, False)
    loc_z, ori_z = _engine_logits(model, ds)
    state, outs = _state_bits(model), _output_bits(model)
    plain = pr.predict(model, ds)
    assert all(np.array_equal(a, b) for a, b in zip(outs, _output_bits(model)))          # (the same last batch: the same bits)
    _same(plain, pr.predict(model, ds, calibration=None), PKEYS)
    _same(plain, pr.predict(model, ds, calibration=Cal.Calibration(ori_beta=1.0)), PKEYS)
    _same(plain, pr.predict(model, ds, calibration=Cal.Calibration(ori_beta=1.0, loc_beta=1.0, k_ori=512, k_loc=64)), PKEYS)
    cal = Cal.Calibration(ori_beta=2.0, loc_beta=0.5)
    p = pr.predict(model, ds, calibration=cal)
    assert all(np.array_equal(a, b) for a, b in zip(outs, _output_bits(model))), "the engine's outputs were scaled"
    z2, l2 = Cal.scale32(ori_z, 2.0), Cal.scale32(loc_z, 0.5)                             # (exact in fp32: powers of two)
    assert np.array_equal(z2.astype(np.float64), 2.0 * ori_z.astype(np.float64))
    peak = P.peak(z2)
    assert np.all(np.abs(p.ori_peak - peak) <= 1e-9 * peak) and np.all(p.ori_peak > plain.ori_peak)
    hq = np.ascontiguousarray(ds.ori_histogram_map, dtype=np.float32)
    A, Mm = P.scatter(z2, hq)
    ratio, excl = P.gate_decode(p.q_est, ori_z.shape[1], A, Mm)
    print("q_est observed / bound", ratio, "excluded", int(excl.sum()))
    assert not excl.any() and ratio <= 1
    print("angle to the plain estimate [rad]", P.angle(p.q_est, plain.q_est))
    assert not np.array_equal(p.q_est, plain.q_est)
    loc_ref, lpeak = P.loc_softmax(l2, np.asarray(ds.histogram_3D_map, dtype=np.float64))
    assert np.all(np.abs(p.loc_est - loc_ref) <= 1e-9 * np.abs(loc_ref)) and np.all(np.abs(p.loc_peak - lpeak) <= 1e-9 * lpeak)
    assert np.all(p.loc_peak < plain.loc_peak)
    only_ori = pr.predict(model, ds, calibration=Cal.Calibration(ori_beta=2.0))
    assert np.array_equal(only_ori.q_est, p.q_est) and np.array_equal(only_ori.loc_est, plain.loc_est)
    # evaluate: the same estimate, its own errors, a fifth line
    (workdir / "e0").mkdir(); (workdir / "e1").mkdir()
    capsys.readouterr()
    e0 = ev.evaluate(model, ds, out_dir=str(workdir / "e0"))
    lines0 = capsys.readouterr().out.splitlines()
    e = ev.evaluate(model, ds, out_dir=str(workdir / "e1"), calibration=cal)
    lines = capsys.readouterr().out.splitlines()
    assert np.array_equal(e.q_est, p.q_est) and np.array_equal(e.loc_est, p.loc_est)
    assert np.array_equal(e0.q_est, plain.q_est) and len(lines0) == 4
    assert len(lines) == 5 and lines[:4] == ev.summary_lines(e.means()) and lines[4] == cal.line()
    assert lines[4] == "Calibration: orientation T = 0.5 (beta 2.0), location T = 2.0 (beta 0.5)"
    q_gt = np.stack([np.asarray(ds.load_quaternion(i), dtype=np.float64) for i in ds.image_ids])
    loc_gt = np.stack([np.asarray(ds.load_location(i), dtype=np.float64) for i in ds.image_ids])
    from test_views_gpu import _close, _errors
    for i in range(7):                                                        # the errors are those of the calibrated estimate
        for got, want in zip((e.loc_err[i], e.ori_err[i], e.esa[i], e.dist[i]), _errors(e.loc_est[i], e.q_est[i], loc_gt[i], q_gt[i])):
            assert _close(got, want), (i, got, want)
    assert np.array_equal(e.ori_encoded_err, e0.ori_encoded_err) and np.array_equal(e.loc_encoded_err, e0.loc_encoded_err)
    # multimodal and views run on the scaled logits
    mm = pr.predict(model, ds, multimodal=True, calibration=cal)
    assert np.array_equal(mm.q_est, p.q_est) and mm.modes.shape == (7, 3, 4)
    from ursonet_amd import pose
    ref_modes = pose.fit_orientation_modes(z2, ds.ori_histogram_map, (cfg.BETA / cfg.ORI_BINS_PER_DIM) ** 2 / 12, 5, 4)
    assert np.array_equal(mm.n_modes, ref_modes[4])
    views = [[0.0, 0.0, 0.0]]
    v0, v1 = pr.predict(model, ds, views=views), pr.predict(model, ds, views=views, calibration=cal)
    assert np.array_equal(v0.q_est, plain.q_est) and np.array_equal(v1.q_est, p.q_est) and np.array_equal(v1.loc_est, p.loc_est)
    after = _state_bits(model)
    assert np.array_equal(state[0], after[0]) and np.array_equal(state[1], after[1])
    # refusals that need the model
    with pytest.raises(ValueError, match="fitted on a ori head of 4096 bins, the model's has 512"):
        pr.predict(model, ds, calibration=Cal.Calibration(ori_beta=2.0, k_ori=4096))
    cfg_r, model_r, ds_r = _setup(workdir, True)
    with pytest.raises(ValueError, match="loc_beta = 0.5, but the model's location head is a regression head"):
        ev.evaluate(model_r, ds_r, out_dir=str(workdir), verbose=0, calibration=cal)
