"""Occlusion sensitivity on the GPU: urso_occl_fill_u8, urso_occl_splat and urso_heat_overlay_u8 byte for byte / bit for bit against
their NumPy statements (ursonet_amd.explain.occlude_host / splat64 / overlay_host), urso_occl_score against score64 under the
operation-counted bounds of tests/occlref.py, its independence of position and batch size, and explain() end to end on the small model
of tests/test_calibrate_gpu.py against a restatement that builds the same chunks on the host.  Buffers are 0xA5 / NaN wherever a kernel
must not write, with guard rows."""
import numpy as np
import pytest
import torch

import occlref as R
from ursonet_amd import explain as X
from util import make_config

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD = 0xA5


def _dev(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a if dt is None else np.asarray(a, dtype=dt))).cuda()


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize]).copy()


def _same(a, b):
    """Equal bit for bit; a NaN equals a NaN (the payload of a NaN an operation makes is the hardware's own)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a[~nan]), _bits(b[~nan]))


# ------------------------------------------------------------------ fill
def _rect_list(H, W):
    """Empty, full frame, one pixel, rects touching each border, rects whose edges fall inside a 16-byte vector, rects reaching past
    the frame (clamped), an inverted one."""
    return [(0, 0, 0, 0), (0, 0, H, W), (H // 2, W // 2, H // 2 + 1, W // 2 + 1), (0, 0, 2, 3), (H - 2, W - 3, H, W), (1, 0, H - 1, 1),
            (1, W - 1, H - 1, W), (1, 1, H - 1, min(W, 6)), (0, 2, H, 3), (H - 2, W - 2, H + 10, W + 10), (-3, -3, 2, 2), (3, 3, 1, 1),
            (2, W // 3, 3, W // 3 + 7), (-9, -9, -1, -1)]


@pytest.mark.parametrize("B", [3, 32])
@pytest.mark.parametrize("shape", [(5, 7, 3), (8, 16, 1), (16, 21, 4), (128, 192, 3)])
def test_fill_is_occlude_host(shape, B):
    from ursonet_amd import hip
    H, W, Cc = shape
    N = H * W * Cc
    rng = np.random.default_rng([H, W, Cc, B])
    frame = rng.integers(0, 256, size=shape, dtype=np.uint8)
    fill = (9, 200, 31, 77)
    rects = _rect_list(H, W)
    while len(rects) < 2 * B:
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        rects.append((y, x, y + int(rng.integers(1, H + 1)), x + int(rng.integers(1, W + 1))))
    for mis in (0, 5):                                                        # the batch on a 16-byte boundary, and 5 bytes behind one
        sstore = torch.full((N + 32,), GUARD, dtype=torch.uint8, device="cuda")
        src = sstore[16 + (3 if mis else 0):][:N].view(H, W, Cc)
        src.copy_(_dev(frame))
        for n in sorted({1, B - 1, B}):
            for start in range(0, len(rects) if B == 3 else 1, n):
                use = (rects[start:] + rects)[:n]
                ostore = torch.full(((B + 2) * N + 32,), GUARD, dtype=torch.uint8, device="cuda")
                lead = N + 16 - (ostore.data_ptr() + N) % 16 + mis
                out = ostore[lead:lead + B * N].view(B, H, W, Cc)
                assert out.data_ptr() % 16 == mis
                # the rect table holds rows behind n that must not be read into anything: made huge
                rd = _dev(np.array(use + [(0, 0, 1 << 20, 1 << 20)], dtype=np.int32))
                hip.occl_fill_u8(src, rd, fill, out, n)
                torch.cuda.synchronize()
                host = ostore.cpu().numpy()
                got = host[lead:lead + B * N].reshape(B, H, W, Cc)
                assert np.array_equal(got[:n], X.occlude_host(frame, use, fill)), (shape, B, n, start, mis)
                assert np.all(got[n:] == GUARD) and np.all(host[:lead] == GUARD) and np.all(host[lead + B * N:] == GUARD), "rows >= n or a guard was written"
        back, off = sstore.cpu().numpy(), 16 + (3 if mis else 0)
        assert np.array_equal(back[off:off + N].reshape(shape), frame) and np.all(back[:off] == GUARD) and np.all(back[off + N:] == GUARD), "the source was written"


def test_fill_refuses_a_source_inside_the_batch():
    from ursonet_amd import hip
    out = torch.zeros((3, 5, 7, 3), dtype=torch.uint8, device="cuda")
    rd = _dev(np.zeros((1, 4), dtype=np.int32))
    with pytest.raises(hip.UrsoHipError, match="src lies inside out"):
        hip.occl_fill_u8(out[1], rd, (0, 0, 0, 0), out, 1)


# ------------------------------------------------------------------ score
class _Score(object):
    """The device buffers of one urso_occl_score launch, NaN wherever the kernel must neither read nor write: logits in rows ld apart,
    `mis` floats behind a 16-byte boundary (the baseline's one more); tables with rows in front of row0 and behind row0 + n."""

    def __init__(self, B, n, row0, pad=3, mis=1):
        self.B, self.n, self.row0, self.pad, self.mis = B, n, row0, pad, mis
        self.rows = row0 + B + 1
        self.out = torch.full((self.rows, X.COLS), NAN, dtype=torch.float64, device="cuda")
        self.dec = torch.full((self.rows, X.DEC_COLS), NAN, dtype=torch.float64, device="cuda")

    def head(self, z0, z):
        K, ld = len(z0), len(z0) + self.pad
        store = torch.full((self.B * ld + 8,), NAN, dtype=torch.float32, device="cuda")
        zb = store[self.mis:self.mis + self.B * ld].view(self.B, ld)[:, :K]
        zb[:self.n] = _dev(z)
        s0 = torch.full((K + 8,), NAN, dtype=torch.float32, device="cuda")
        b0 = s0[(self.mis + 1) % 4:][:K]
        b0.copy_(_dev(z0))
        return b0, zb

    def run(self, dec0, dec, ori=None, loc=None):
        from ursonet_amd import hip
        self.dec[self.row0:self.row0 + self.n] = _dev(dec)
        d0 = _dev(dec0)
        kw = {}
        if ori is not None:
            kw["ori_z0"], kw["ori_z"] = self.head(*ori)
        if loc is not None:
            kw["loc_z0"], kw["loc_z"] = self.head(*loc)
        hip.occl_score(self.B, self.n, self.row0, d0, self.dec, self.out, **kw)
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        keep = np.ones(self.rows, dtype=bool)
        keep[self.row0:self.row0 + self.n] = False
        assert np.all(np.isnan(out[keep])), "a row outside [row0, row0 + n) was written"
        return out[self.row0:self.row0 + self.n]


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("K", R.KS)
def test_score_against_the_float64_statement(K, scale):
    """Every case of occlref.head_cases as the orientation head and as the location head, at B = 5, n = 4, row0 = 2, rows K + 3 apart and
    off the 16-byte boundary: KL, TV and DROP within occlref's bounds, ARGMAX, the +inf and the NaN rows exact, the row equal to the
    baseline exact zeros; the other head's columns and the rows outside keep their NaN."""
    dec0, dec = R.dec_rows(R.N, seed=K)
    for name, z0, z in R.head_cases(K, scale):
        for head, lo in (("ori", X.ORI_KL), ("loc", X.LOC_KL)):
            got = _Score(R.B, R.N, R.ROW0).run(dec0, dec, **{head: (z0, z)})
            other = X.LOC_KL if head == "ori" else X.ORI_KL
            assert np.all(np.isnan(got[:, other:other + 4])), "an absent head's columns were written"
            fig = dict(R.check_head(got[:, lo:lo + 4], z0, z), **R.check_pose(got, dec0, dec))
            print("K=%d scale=%g %s %s observed / bound:" % (K, scale, name, head), {k: "%.3g" % v for k, v in fig.items()})
            assert got[3, lo:lo + 3].tolist() == [0, 0, 0], "the row equal to the baseline gives exact zeros"
            assert got[0, X.D_LOC] == 0, "the baseline's own pose"
            for k, v in fig.items():
                assert v <= 1, (K, scale, name, head, k, fig)


def test_score_without_logits_writes_the_pose_columns_only():
    dec0, dec = R.dec_rows(R.N, seed=1)
    got = _Score(R.B, R.N, R.ROW0).run(dec0, dec)
    assert np.all(np.isnan(got[:, X.ORI_KL:])) and np.all(np.isfinite(got[:, :X.ORI_KL]))
    fig = R.check_pose(got, dec0, dec)
    assert max(fig.values()) <= 1, fig
    _, z0, z = R.head_cases(64, 1.0)[0]
    _, l0, lz = R.head_cases(63, 30.0)[1]
    both = _Score(R.B, R.N, R.ROW0).run(dec0, dec, ori=(z0, z), loc=(l0, lz))       # two heads of different K in one launch
    assert np.array_equal(_bits(both[:, :X.ORI_KL]), _bits(got[:, :X.ORI_KL]))
    assert max(R.check_head(both[:, X.ORI_KL:X.LOC_KL], z0, z).values()) <= 1 and max(R.check_head(both[:, X.LOC_KL:], l0, lz).values()) <= 1


@pytest.mark.parametrize("K", [63, 257, 4096])
def test_score_is_a_function_of_the_row_and_the_baseline_alone(K):
    """Two launches give equal bits; a row at (B, n, row0) = (5, 4, 2) in padded, misaligned rows and the same row alone at (1, 1, 0),
    packed, on a 16-byte boundary or two floats off, give equal bits -- the NaN row and the +inf row included."""
    dec0, dec = R.dec_rows(R.N, seed=K)
    for name, z0, z in R.head_cases(K, 30.0):
        first = _bits(_Score(R.B, R.N, R.ROW0).run(dec0, dec, ori=(z0, z), loc=(z0, z)))
        again = _bits(_Score(R.B, R.N, R.ROW0).run(dec0, dec, ori=(z0, z), loc=(z0, z)))
        assert np.array_equal(first, again) and np.array_equal(first[:, X.ORI_KL:X.LOC_KL], first[:, X.LOC_KL:])
        for r in range(R.N):
            for mis in (0, 2):
                alone = _bits(_Score(1, 1, 0, pad=0, mis=mis).run(dec0, dec[r:r + 1], ori=(z0, z[r:r + 1]), loc=(z0, z[r:r + 1])))
                assert np.array_equal(first[r], alone[0]), (name, r, mis)


# ------------------------------------------------------------------ splat
def _splat(scores, cols, rects, window):
    from ursonet_amd import hip
    y0, x0, y1, x1 = window
    M, h, w = len(cols), y1 - y0, x1 - x0
    store = torch.full((M * h * w + 16,), 777.0, dtype=torch.float64, device="cuda")
    out = store[8:8 + M * h * w].view(M, h, w)
    hip.occl_splat(_dev(scores), cols, _dev(np.asarray(rects, dtype=np.int32).reshape(-1, 4)), window, out)
    torch.cuda.synchronize()
    host = store.cpu().numpy()
    assert np.all(host[:8] == 777.0) and np.all(host[8 + M * h * w:] == 777.0), "a guard was written"
    return host[8:8 + M * h * w].reshape(M, h, w)


@pytest.mark.parametrize("cols", [[5], [6, 0, 3]])
@pytest.mark.parametrize("window,patch,stride", [((0, 0, 6, 9), 4, 2), ((3, 5, 10, 12), 3, 2), ((1, 2, 9, 7), (2, 5), (1, 3)), ((0, 0, 7, 7), 64, 64),
                                                 ((3, 5, 10, 12), 1, 1), ((0, 0, 37, 50), 8, 5)])
def test_splat_is_splat64(window, patch, stride, cols):
    rects = X.occlusion_rects(window, patch, stride)
    rng = np.random.default_rng(len(rects))
    scores = rng.normal(size=(len(rects), 7)) * 10 ** rng.uniform(-3, 3, size=(len(rects), 7))
    scores[len(rects) // 2, cols[0]] = np.nan
    scores[0, cols[-1]] = np.inf
    got = _splat(scores, cols, rects, window)
    ref = X.splat64(scores, cols, rects, window)
    assert _same(got, ref) and not np.all(np.isfinite(got)) and not np.all(np.isnan(got))


@pytest.mark.parametrize("cols", [[1], [2, 0, 1]])
def test_splat_leaves_uncovered_pixels_nan(cols):
    window = (2, 3, 9, 14)
    rects = [(2, 3, 4, 6), (3, 4, 6, 8), (0, 0, 2, 3), (8, 13, 20, 20), (5, 5, 5, 9), (4, 10, 7, 11), (-5, -5, 30, 4)]
    scores = np.arange(21, dtype=np.float64).reshape(7, 3) / 7.0
    got = _splat(scores, cols, rects, window)
    ref = X.splat64(scores, cols, rects, window)
    assert _same(got, ref)
    cover = np.zeros((7, 11), dtype=bool)
    for a, b, c, d in rects:
        cover[max(a - 2, 0):max(c - 2, 0), max(b - 3, 0):max(d - 3, 0)] = True
    assert np.array_equal(np.isnan(got[0]), ~cover) and (~cover).any()
    none = _splat(scores, cols, [(0, 0, 2, 3), (9, 3, 12, 14)], window)                # no patch reaches the window
    assert np.all(np.isnan(none))


# ------------------------------------------------------------------ overlay
@pytest.mark.parametrize("alpha", [0, 1, 128, 256])
def test_overlay_is_overlay_host(alpha):
    from ursonet_amd import hip
    rng = np.random.default_rng(alpha)
    img = rng.integers(0, 256, size=(12, 15, 3), dtype=np.uint8)
    h, w, lo, hi = 7, 9, -1.0, 2.0
    scale = 255.0 / (hi - lo)
    heat = rng.uniform(lo, hi, size=(h, w))
    heat[0, 0], heat[0, 1], heat[0, 2], heat[0, 3], heat[0, 4] = np.nan, lo, hi, lo - 5, hi + 5
    heat[1, 0], heat[1, 1], heat[1, 2] = np.inf, -np.inf, lo + 0.5 / scale                # the last: a tie of rint, up to a rounding
    lut = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
    d = _dev(img)
    win = d[2:2 + h, 3:3 + w]
    assert win.stride(0) == 45 and not win.is_contiguous()
    hip.heat_overlay_u8(_dev(heat), lo, scale, _dev(lut), alpha, win)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    want = img.copy()
    want[2:2 + h, 3:3 + w] = X.overlay_host(img[2:2 + h, 3:3 + w], heat, lo, scale, lut, alpha)
    assert np.array_equal(got, want), "the window differs from overlay_host, or a pixel outside it was written"
    assert np.array_equal(got[2, 3], img[2, 3]), "a NaN leaves the pixel"
    if alpha == 256:
        assert np.array_equal(got[2, 4], lut[0]) and np.array_equal(got[2, 5], lut[255]) and np.array_equal(got[2, 6], lut[0]) and np.array_equal(got[2, 7], lut[255])
    if alpha == 0:
        assert np.array_equal(got, img)


# ------------------------------------------------------------------ end to end
_CACHE = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("explain")


def _setup(workdir, regress_loc):
    """(cfg, model, dataset): the model of tests/test_calibrate_gpu.py -- an inference ResNet-18 at 128 x 192 in fp32 with the soft
    orientation head (8^3 bins), engine batch 3 -- and 7 synthetic images."""
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
    _CACHE[regress_loc] = (cfg, model, ds)
    return _CACHE[regress_loc]


def _state_bits(model):
    eng = model._engine
    return _bits(eng.flat_w), _bits(eng.flat_stats)


def _output_bits(model):
    loc, ori = model._engine.outputs()
    return _bits(loc.contiguous()), _bits(ori.contiguous())


def _restate(model, ds, ids, patch, stride, fill, calibration=None):
    """explain()'s chunks built on the host: per image the rows [empty rect] + rects through occlude_host into a host batch that keeps,
    as explain()'s scratch batch does, the rows a tail chunk leaves out; each chunk through PosePass.run / heads / decode_into at the
    same batch composition.  -> per image (dec [P + 1, DEC_COLS], ori logits [P + 1, K] or None, loc logits or None, rects, frame)."""
    from ursonet_amd import hip, utils
    from ursonet_amd.infer import PosePass
    cfg = model.config
    ps = PosePass(model, ds, scatter=True, who="explain", calibration=calibration)
    B = ps.B
    batch = None
    out = []
    for i in ids:
        frame = ds.load_image(i)
        scale, _size, _pads, window = utils.resize_geometry(frame.shape[0], frame.shape[1], cfg.IMAGE_MIN_DIM, cfg.IMAGE_MAX_DIM, cfg.IMAGE_MIN_SCALE,
                                                            cfg.IMAGE_RESIZE_MODE)
        assert scale == 1 and tuple(window) == (0, 0) + frame.shape[:2], "the synthetic frames are the model's size: the frame is the batch row"
        rects = X.occlusion_rects(window, patch, stride)
        rows = np.concatenate([np.array([X.EMPTY_RECT], dtype=np.int32), rects])
        if batch is None:
            batch = np.zeros((B,) + frame.shape, dtype=np.uint8)
        dec = ps.table(len(rows), hip.DEC_COLS)
        zs, ls = [], []
        for r0 in range(0, len(rows), B):
            n = min(B, len(rows) - r0)
            batch[:n] = X.occlude_host(frame, rows[r0:r0 + n], fill)
            ps.run(_dev(batch))
            heads = ps.heads(n)
            ps.decode_into(dec, n, r0, heads)
            if ps.soft:
                zs.append(heads[3][:n].cpu().numpy().copy())
            if ps.loc_class:
                ls.append(heads[0][:n].cpu().numpy().copy())
        out.append((dec.cpu().numpy(), np.concatenate(zs) if zs else None, np.concatenate(ls) if ls else None, rects, frame))
    return out


@pytest.mark.parametrize("regress_loc", [True, False])
def test_explain_end_to_end(workdir, regress_loc):
    """2 images, patch 32, stride 32 at 128 x 192 and engine batch 3: 24 patches, 25 rows in 9 passes with a tail of one."""
    cfg, model, ds = _setup(workdir, regress_loc)
    ids = [4, 1]
    fill = tuple(int(v) for v in np.rint(cfg.MEAN_PIXEL).astype(np.uint8))
    before = _state_bits(model)
    shots = []
    res = X.explain(model, ds, image_ids=ids, patch=32, stride=32, render=True, sink=lambda i, name, a: shots.append((i, name, a.copy())))
    outputs = _output_bits(model)
    after = _state_bits(model)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "the weights or the statistics changed"
    assert res.image_ids.tolist() == ids and res.patches.tolist() == [24, 24] and res.passes.tolist() == [9, 9] and res.pictures is None
    assert res.window.tolist() == [[0, 0, 128, 192]] * 2 and res.loc_est.shape == (2, 3) and res.q_est.shape == (2, 4)
    names = {"d_ori", "d_loc", "ori_kl", "ori_tv", "ori_drop"} | (set() if regress_loc else {"loc_kl", "loc_tv", "loc_drop"})
    ref = _restate(model, ds, ids, 32, 32, fill)
    assert np.array_equal(_output_bits(model)[0], outputs[0]) and np.array_equal(_output_bits(model)[1], outputs[1]), \
        "the restatement's last pass is explain()'s: the engine's output buffers hold the same bits"
    lut = X.heat_lut()
    for k, (dec, z, lz, rects, frame) in enumerate(ref):
        assert np.array_equal(res.rects[k], rects) and res.scores[k].shape == (24, X.COLS) and set(res.maps[k]) == names
        assert np.array_equal(_bits(res.loc_est[k]), _bits(dec[0, X.DEC_LOC_EST:X.DEC_LOC_EST + 3])), "LOC_EST of the baseline, bit for bit"
        assert np.array_equal(_bits(res.q_est[k]), _bits(dec[0, X.DEC_Q_EST:X.DEC_Q_EST + 4])), "Q_EST of the baseline, bit for bit"
        table = np.concatenate([res.baseline_scores[k][None], res.scores[k]])
        assert R.no_underflow(z) and (lz is None or R.no_underflow(lz))
        fig = dict(R.check_pose(table, dec[0], dec), **{"ori_" + n: v for n, v in R.check_head(table[:, X.ORI_KL:X.LOC_KL], z[0], z).items()})
        if lz is not None:
            fig.update({"loc_" + n: v for n, v in R.check_head(table[:, X.LOC_KL:], lz[0], lz).items()})
        else:
            assert np.all(np.isnan(table[:, X.LOC_KL:])), "a regressed location has no PMF columns"
        print("image %d regress_loc=%s observed / bound:" % (ids[k], regress_loc), {n: "%.3g" % v for n, v in fig.items()})
        for n, v in fig.items():
            assert v <= 1, (k, n, fig)
        base = res.baseline_scores[k]
        assert base[X.ORI_KL:X.ORI_KL + 3].tolist() == [0, 0, 0] and base[X.D_LOC] == 0 and base[X.ORI_ARGMAX] == int(np.argmax(z[0]))
        assert lz is None or base[X.LOC_KL:X.LOC_KL + 3].tolist() == [0, 0, 0]
        cols = [c for n, c in X.MAP_COLUMNS if n in names]
        maps = X.splat64(res.scores[k], cols, rects, res.window[k])
        for m, (n, c) in enumerate((n, c) for n, c in X.MAP_COLUMNS if n in names):
            assert _same(res.maps[k][n], maps[m]), n
            assert _same(res.maps[k][n][:32, :32], np.full((32, 32), 0.0 + res.scores[k][0, c])), "stride = patch: a patch's pixels hold its score"
        rng = X.heat_range(res.maps[k]["d_ori"])
        i, name, pic = shots[k]
        assert (i, name) == (k, "heat") and pic.dtype == np.uint8 and pic.shape == (128, 192, 3)
        want = frame if rng is None else X.overlay_host(frame, res.maps[k]["d_ori"], rng[0], rng[1], lut, 128)
        assert np.array_equal(pic, want), "the picture is overlay_host on the frame's window"
        peak, centroid, off = X.summaries(res.maps[k]["d_ori"], None)
        assert np.array_equal(res.peak_xy[k], peak) and np.array_equal(res.centroid_xy[k], centroid, equal_nan=True)
        assert np.isfinite(res.centroid_offset[k]) or np.isnan(centroid).any()
    # nr_images takes the first of dataset.image_ids; pictures without a sink come back in the result
    few = X.explain(model, ds, nr_images=1, patch=(64, 96), stride=(64, 96), render="ori_tv", alpha=256)
    assert few.image_ids.tolist() == [int(ds.image_ids[0])] and few.patches.tolist() == [4] and few.passes.tolist() == [2]
    rng = X.heat_range(few.maps[0]["ori_tv"])
    assert rng is not None and np.array_equal(few.pictures[0], X.overlay_host(ds.load_image(ds.image_ids[0]), few.maps[0]["ori_tv"], rng[0], rng[1], lut, 256))


def test_explain_with_a_calibration(workdir):
    """A calibration changes the PMF columns (and the soft-argmax orientation) and leaves D_LOC of a regressed location as it is; the
    engine's output buffers are not written by it; the scores equal the restatement's under the same calibration."""
    from ursonet_amd.calibrate import Calibration
    cfg, model, ds = _setup(workdir, True)
    ids = [4]
    fill = tuple(int(v) for v in np.rint(cfg.MEAN_PIXEL).astype(np.uint8))
    plain = X.explain(model, ds, image_ids=ids, patch=32, stride=32)
    outputs = _output_bits(model)
    before = _state_bits(model)
    cal = Calibration(ori_beta=2.5)
    hot = X.explain(model, ds, image_ids=ids, patch=32, stride=32, calibration=cal)
    after = _state_bits(model)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(_output_bits(model)[0], outputs[0]) and np.array_equal(_output_bits(model)[1], outputs[1]), "the engine's outputs were written"
    assert np.array_equal(_bits(hot.scores[0][:, X.D_LOC]), _bits(plain.scores[0][:, X.D_LOC])) and np.array_equal(_bits(hot.loc_est), _bits(plain.loc_est))
    assert not np.array_equal(hot.scores[0][:, X.ORI_KL], plain.scores[0][:, X.ORI_KL]) and not np.array_equal(hot.scores[0][:, X.ORI_TV], plain.scores[0][:, X.ORI_TV])
    (dec, z, _lz, _rects, _frame), = _restate(model, ds, ids, 32, 32, fill, calibration=cal)
    table = np.concatenate([hot.baseline_scores[0][None], hot.scores[0]])
    fig = dict(R.check_pose(table, dec[0], dec), **R.check_head(table[:, X.ORI_KL:X.LOC_KL], z[0], z))
    print("calibrated observed / bound:", {n: "%.3g" % v for n, v in fig.items()})
    assert max(fig.values()) <= 1, fig
    assert np.array_equal(_bits(hot.q_est[0]), _bits(dec[0, X.DEC_Q_EST:X.DEC_Q_EST + 4]))
