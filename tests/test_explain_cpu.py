"""Occlusion sensitivity without a GPU (explain(), ursonet_amd/explain.py): the patch grid's properties, the four NumPy statements of the
kernels (occlude_host, score64, splat64, overlay_host), the premises of tests/occlref.py's cases, every refusal of explain() before
torch, the engine or the library is touched, the surface of liburso_explain.so against header and bindings, and the four entry points'
argument checks (they run before any HIP call)."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import occlref as R
from libsurface import header_symbols
from ursonet_amd import explain as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_explain.h")
NAMES = {"urso_occl_fill_u8", "urso_occl_score", "urso_occl_splat", "urso_heat_overlay_u8"}
WINDOWS = [(0, 0, 128, 192), (3, 5, 10, 12), (0, 0, 5, 40), (2, 1, 40, 6), (7, 7, 9, 10), (0, 0, 1, 1)]
GRIDS = [(32, 32), (32, None), (8, 1), (8, 8), (8, 3), (8, 5), ((8, 16), (3, 7)), (1, 1), (64, 64), ((3, 50), (2, 9))]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------ the patch grid
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("patch,stride", GRIDS)
def test_occlusion_rects_properties(window, patch, stride):
    y0, x0, y1, x1 = window
    rects = X.occlusion_rects(window, patch, stride)
    assert rects.dtype == np.int32 and rects.ndim == 2 and rects.shape[1] == 4 and len(rects) >= 1
    ph, pw = (patch, patch) if np.ndim(patch) == 0 else patch
    sh, sw = (max(1, ph // 2), max(1, pw // 2)) if stride is None else ((stride, stride) if np.ndim(stride) == 0 else stride)
    cover = np.zeros((y1 - y0, x1 - x0), dtype=int)
    for a, b, c, d in rects:
        assert y0 <= a < c <= y1 and x0 <= b < d <= x1, "a rect leaves the window or is empty"
        assert c - a == min(ph, y1 - y0) and d - b == min(pw, x1 - x0), "every rect has the patch's size, clipped to the window"
        cover[a - y0:c - y0, b - x0:d - x0] += 1
    assert cover.min() >= 1, "a window pixel is not covered"
    keys = [(int(r[0]), int(r[1])) for r in rects]
    assert keys == sorted(set(keys)), "row-major and unique"
    ys, xs = sorted({k[0] for k in keys}), sorted({k[1] for k in keys})
    assert len(keys) == len(ys) * len(xs)
    for pos, a, b, p, s in ((ys, y0, y1, ph, sh), (xs, x0, x1, pw, sw)):
        assert pos[0] == a and pos[-1] == (a if p >= b - a else b - p), "the last position is b - p"
        steps = np.diff(pos)
        assert np.all(steps[:-1] == s) and (len(steps) == 0 or 0 < steps[-1] <= s)


def test_occlusion_rects_counts_and_refusals():
    assert len(X.occlusion_rects((0, 0, 128, 192), 32, 32)) == 24
    assert len(X.occlusion_rects((0, 0, 128, 192), 32)) == 7 * 11                      # stride 16
    assert X.occlusion_rects((3, 5, 10, 12), 64).tolist() == [[3, 5, 10, 12]]
    assert X.occlusion_rects((0, 0, 10, 10), 4, 3)[:, 0].max() == 6 and X.occlusion_rects((0, 0, 10, 10), 1).shape == (100, 4)
    for bad in (0, -1, (4,), (4, 0), "a", 2.5, None, True, (1, 2, 3)):
        with pytest.raises(ValueError, match="patch is an int or a pair"):
            X.occlusion_rects((0, 0, 8, 8), bad)
    for bad in (0, (3, -2), 1.5):
        with pytest.raises(ValueError, match="stride is an int or a pair"):
            X.occlusion_rects((0, 0, 8, 8), 4, bad)
    with pytest.raises(ValueError, match="is empty"):
        X.occlusion_rects((4, 4, 4, 9), 4)


# ------------------------------------------------------------------ the statements
def test_occlude_host():
    rng = np.random.default_rng(0)
    for shape in ((5, 7, 3), (8, 16, 1), (6, 5, 4)):
        H, W, Cc = shape
        frame = rng.integers(0, 256, size=shape, dtype=np.uint8)
        rects = [(0, 0, 0, 0), (3, 3, 3, 5), (2, 4, 1, 6), (0, 0, H, W), (-3, -2, H + 4, W + 9), (1, 2, 3, 4), (H - 1, W - 1, H + 5, W + 5), (-5, -5, -1, -1)]
        fill = (9, 200, 31, 77)
        out = X.occlude_host(frame, rects, fill)
        assert out.shape == (len(rects),) + shape and out.dtype == np.uint8
        for j in (0, 1, 2, 7):
            assert np.array_equal(out[j], frame), "an empty rect copies"
        for j in (3, 4):
            assert np.array_equal(out[j], np.broadcast_to(np.array(fill[:Cc], dtype=np.uint8), shape)), "a full-frame rect gives the fill"
        want = frame.copy()
        want[1:3, 2:4] = fill[:Cc]
        assert np.array_equal(out[5], want)
        want = frame.copy()
        want[H - 1, W - 1] = fill[:Cc]
        assert np.array_equal(out[6], want), "a rect is clamped to the frame"


def test_score64_rules():
    dec0, dec = R.dec_rows(4)
    z0 = np.array([0.5, -1.0, 2.0, 0.25], dtype=np.float32)
    z = np.stack([z0, z0[::-1], np.array([0.5, -np.inf, 2.0, 0.25], dtype=np.float32), np.array([0.5, np.nan, 2.0, 0.25], dtype=np.float32)])
    s = X.score64(dec0, dec, ori_z0=z0, ori_z=z)
    assert s.shape == (4, X.COLS) and np.all(np.isnan(s[:, X.LOC_KL:])), "an absent head stays NaN"
    assert s[0, X.ORI_KL] == 0 and s[0, X.ORI_TV] == 0 and s[0, X.ORI_DROP] == 0 and s[0, X.ORI_ARGMAX] == 2, "identical rows give exact zeros"
    assert s[0, X.D_LOC] == 0 and s[0, X.D_ORI] <= R.angle_interval(dec0[3:7], dec0[3:7])[1]
    assert s[1, X.D_ORI] <= R.angle_interval(dec0[3:7], dec0[3:7])[1], "a quaternion and its antipode are one rotation"
    assert s[1, X.ORI_KL] > 0 and 0 < s[1, X.ORI_TV] <= 1 and s[1, X.ORI_ARGMAX] == 1 and s[1, X.ORI_DROP] > 0
    assert np.isposinf(s[2, X.ORI_KL]) and 0 < s[2, X.ORI_TV] <= 1, "p0 > 0 where p = 0: +inf"
    assert np.all(np.isnan(s[3, X.ORI_KL:X.ORI_KL + 4])) and np.isfinite(s[3, X.D_ORI]), "a NaN row: four NaNs, the pose columns stay"
    hole = z0.copy()
    hole[1] = -np.inf
    back = X.head64(hole, z0)                                                      # p0 == 0 contributes exactly 0
    p0, lp0 = X._pmf64(hole)
    p1, lp1 = X._pmf64(z0)
    use = [0, 2, 3]
    assert np.isfinite(back[0]) and abs(back[0] - np.sum(p0[use] * (lp0[use] - lp1[use]))) <= 1e-15
    assert X.head64(hole, hole)[:3].tolist() == [0, 0, 0] and X.head64(hole, hole)[3] == 2
    assert X.head64(np.float32([3.0]), np.float32([-7.0])).tolist() == [0, 0, 0, 0], "K = 1"
    assert np.all(np.isnan(X.head64(np.float32([-np.inf, -np.inf]), z0[:2]))) and np.all(np.isnan(X.head64(z0[:2], np.float32([np.inf, 0]))))
    both = X.score64(dec0, dec, ori_z0=z0, ori_z=z, loc_z0=z0[:3], loc_z=z[:, :3])
    assert np.array_equal(bits(both[:, :X.LOC_KL]), bits(s[:, :X.LOC_KL])) and np.all(np.isfinite(both[:2, X.LOC_KL:]))
    # first argmax on ties
    assert X.head64(np.float32([1, 2, 2]), np.float32([5, 5, 1]))[3] == 0
    # a pose: 90 degrees about z, 3-4-12 apart
    a, b = np.zeros(12), np.zeros(12)
    a[3:7], b[3:7], b[0:3] = (0, 0, 0, 1), (0, 0, np.sqrt(0.5), np.sqrt(0.5)), (3, 4, 12)
    ang, dist = X.pose64(a, b)
    assert abs(ang - 90) <= 1e-12 and dist == 13.0


@pytest.mark.parametrize("scale", R.SCALES)
@pytest.mark.parametrize("K", R.KS)
def test_score64_properties_and_the_cases_premises(K, scale):
    for name, z0, z in R.head_cases(K, scale):
        assert R.top_two_differ(z0) and R.top_two_differ(z), (name, "the top two logits tie in some row")
        assert R.no_underflow(z0) and R.no_underflow(z), (name, "an exp of the case underflows")
        for r in range(len(z)):
            out = X.head64(z0, z[r])
            if np.isnan(z[r]).any() or not np.isfinite(z[r].max()):
                assert np.all(np.isnan(out))
                continue
            assert out[0] >= 0 or abs(out[0]) <= R.kl_abs(K, R.lp_max(z0, z[r])), "KL >= 0 up to its bound"
            assert -R.tv_abs(K) <= out[1] <= 1 + R.tv_abs(K) and abs(out[2]) <= 1 and 0 <= out[3] < K and out[3] == int(np.argmax(z[r]))
        same = X.head64(z0, z[3])
        assert same[:3].tolist() == [0, 0, 0] and same[3] == int(np.argmax(z0)), "the row equal to the baseline gives exact zeros"
        if K > 1:
            assert np.isposinf(X.head64(z0, z[1 if name == "plain" else 2])[0]) or K == 2
        fig = R.check_head(np.stack([X.head64(z0, row) for row in z]), z0, z)
        assert max(fig.values()) == 0


@pytest.mark.parametrize("window,patch,stride", [((0, 0, 6, 9), 4, 2), ((3, 5, 10, 12), 3, 2), ((1, 2, 9, 7), (2, 5), (1, 3)), ((0, 0, 7, 7), 64, 64)])
def test_splat64_against_a_double_loop(window, patch, stride):
    rects = X.occlusion_rects(window, patch, stride)
    rng = np.random.default_rng(len(rects))
    scores = rng.normal(size=(len(rects), 5)) * 10 ** rng.uniform(-3, 3, size=(len(rects), 5))
    cols = [4, 0, 2]
    got = X.splat64(scores, cols, rects, window)
    y0, x0, y1, x1 = window
    assert got.shape == (3, y1 - y0, x1 - x0)
    for m, c in enumerate(cols):
        for y in range(y0, y1):
            for x in range(x0, x1):
                s, n = 0.0, 0
                for p, (a, b, e, f) in enumerate(rects):
                    if a <= y < e and b <= x < f:
                        s, n = s + scores[p, c], n + 1
                assert n > 0 and bits(got[m, y - y0, x - x0]) == bits(s / n), (m, y, x)
    # uncovered pixels are NaN; non-finite scores pass through to the pixels their patches cover, and only those
    holes = np.array([(y0, x0, y0 + 1, x0 + 2), (y0 + 1, x0 + 1, y0 + 3, x0 + 3), (y0 - 4, x0 - 4, y0, x0)], dtype=np.int32)
    sc = np.array([[1.0, np.nan], [np.inf, 2.0], [5.0, 5.0]])
    out = X.splat64(sc, [0, 1], holes, window)
    assert out[0, 0, 0] == 1 and np.isnan(out[1, 0, 0]) and np.isposinf(out[0, 1, 1]) and out[1, 1, 1] == 2
    covered = np.zeros(out.shape[1:], dtype=bool)
    covered[0:1, 0:2] = True
    covered[1:3, 1:3] = True
    assert np.array_equal(np.isnan(out[0]), ~covered[:out.shape[1], :out.shape[2]])


def test_overlay_host():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(7, 9, 3), dtype=np.uint8)
    heat = rng.normal(size=(7, 9))
    heat[0, 0], heat[1, 1], heat[2, 2], heat[3, 3] = np.nan, np.inf, -np.inf, 1e300
    lut = X.heat_lut()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and lut[0].tolist() == [0, 0, 0] and lut[255].tolist() == [255, 255, 255]
    assert np.all(np.diff(lut.astype(int).sum(axis=1)) > 0), "the ramp rises"
    lo, scale = X.heat_range(heat)
    fin = heat[np.isfinite(heat)]
    assert lo == fin.min() and scale == 255.0 / (fin.max() - fin.min())
    assert np.array_equal(X.overlay_host(img, heat, lo, scale, lut, 0), img), "alpha 0 leaves the picture"
    full = X.overlay_host(img, heat, lo, scale, lut, 256)
    idx = np.clip(np.rint((heat - lo) * scale), 0, 255)
    for y in range(7):
        for x in range(9):
            if np.isnan(heat[y, x]):
                assert np.array_equal(full[y, x], img[y, x]), "a NaN leaves the pixel"
            else:
                assert np.array_equal(full[y, x], lut[int(idx[y, x])]), "alpha 256 gives the table"
    assert np.array_equal(full[1, 1], lut[255]) and np.array_equal(full[2, 2], lut[0]) and np.array_equal(full[3, 3], lut[255])
    half = X.overlay_host(img, heat, lo, scale, lut, 128)
    y, x = 4, 5
    assert half[y, x].tolist() == [(128 * int(lut[int(idx[y, x]), c]) + 128 * int(img[y, x, c]) + 128) >> 8 for c in range(3)]
    assert X.heat_range(np.full((2, 2), 3.0)) is None and X.heat_range(np.full((2, 2), np.nan)) is None
    # rint is ties-to-even: t = 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    ties = X.overlay_host(np.zeros((1, 3, 3), np.uint8), np.array([[0.5, 1.5, 2.5]]), 0.0, 1.0, lut, 256)
    assert [lut.tolist().index(p.tolist()) for p in ties[0]] == [0, 2, 2]


def test_summaries():
    heat = np.zeros((4, 6))
    heat[1, 2] = heat[3, 0] = 2.0
    peak, centroid, off = X.summaries(heat, (1.0, 5.0))
    assert peak.tolist() == [2, 1] and centroid.tolist() == [1.0, 2.0] and off == 3.0
    peak, centroid, off = X.summaries(np.zeros((2, 2)))
    assert peak.tolist() == [0, 0] and np.all(np.isnan(centroid)) and np.isnan(off)


# ------------------------------------------------------------------ refusals
def test_interface_refuses_before_torch_the_engine_or_the_library():
    code = """
import os, sys
sys.path.insert(0, "tests")
sys.modules["torch"] = None                              # poisoned: any import of torch raises
import numpy as np
import pytest
from util import make_config
from ursonet_amd import explain
class Boom(object):
    def __getattr__(self, name):
        raise AssertionError("touched %s" % name)
class Data(object):
    histogram_3D_map = ori_histogram_map = 1
    def __init__(self, n, dtype=np.uint8, shape=(128, 192, 3)):
        self.image_ids, self.dtype, self.shape, self.loads = list(range(n)), dtype, shape, 0
    def load_image(self, i):
        self.loads += 1
        return np.zeros(self.shape, dtype=self.dtype)
class Model(object):
    _dp, _world = None, 1
    _engine = property(lambda self: Boom().engine)
    def __init__(self, mode="inference", **kw):
        self.mode, self.config = mode, make_config("resnet18", 128, 192, batch=3, **kw)
with pytest.raises(ValueError, match="explain needs a model created in inference mode"):
    explain.explain(Model("training"), Data(2))
with pytest.raises(ValueError, match="orientation classification .* needs dataset.ori_histogram_map"):
    explain.explain(Model(), type("NoMap", (Data,), {"ori_histogram_map": None})(2))
with pytest.raises(ValueError, match="location classification .* needs dataset.histogram_3D_map"):
    explain.explain(Model(regress_loc=False), type("NoMap", (Data,), {"histogram_3D_map": None})(2))
for dtype, shape in ((np.float32, (128, 192, 3)), (np.uint8, (128, 192)), (np.uint8, (128, 192, 1)), (np.uint16, (128, 192, 3))):
    with pytest.raises(ValueError, match="explain occludes uint8 RGB frames; this dataset's frames reach the engine as"):
        explain.explain(Model(), Data(2, dtype, shape))
for bad in (0, -3, (4, 0), (1, 2, 3), "x", 2.5, None):
    with pytest.raises(ValueError, match="explain: patch is an int or a pair"):
        explain.explain(Model(), Data(2), patch=bad)
for bad in (0, (0, 4), "x", 0.5):
    with pytest.raises(ValueError, match="explain: stride is an int or a pair"):
        explain.explain(Model(), Data(2), stride=bad)
for bad in ("median", (1, 2), (1, 2, 256), (1, 2, -1), (1.5, 2, 3), 7, None):
    with pytest.raises(ValueError, match="explain: fill is .mean. or three ints in 0 .. 255"):
        explain.explain(Model(), Data(2), fill=bad)
assert explain._fill_bytes("mean", Model().config) == tuple(int(v) for v in np.rint(Model().config.MEAN_PIXEL).astype(np.uint8))
assert explain._fill_bytes([0, 255, 7], None) == (0, 255, 7)
with pytest.raises(ValueError, match="calibration must be a calibrate.Calibration"):
    explain.explain(Model(), Data(2), calibration=0.5)
with pytest.raises(ValueError, match="explain: render is True or one of the maps d_ori, d_loc, ori_kl, ori_tv, ori_drop of this model"):
    explain.explain(Model(), Data(2), render="loc_kl")
with pytest.raises(ValueError, match="explain: alpha is an int in 0 .. 256"):
    explain.explain(Model(), Data(2), render=True, alpha=257)
with pytest.raises(ValueError, match="explain: lut is a uint8 .256,3. table"):
    explain.explain(Model(), Data(2), render=True, lut=np.zeros((255, 3), np.uint8))
crop = Model()
crop.config.IMAGE_RESIZE_MODE = "crop"
with pytest.raises(ValueError, match="explain: IMAGE_RESIZE_MODE 'crop' has no window to occlude"):
    explain.explain(crop, Data(2))
with pytest.raises(ValueError, match="nr_images must be >= 0"):
    explain.explain(Model(), Data(2), nr_images=-1)
none = explain.explain(Model(), Data(5), nr_images=0)     # nothing to do: no frame is loaded, nothing is touched
assert len(none.image_ids) == 0 and none.maps == [] and none.loc_est.shape == (0, 3) and none.pictures is None
os.environ["WORLD_SIZE"] = "2"
with pytest.raises(ValueError, match="explain is not supported under a data-parallel launcher"):
    explain.explain(Boom(), Boom())
del os.environ["WORLD_SIZE"]
class Ranked(Model):
    _world = 2
with pytest.raises(ValueError, match="explain is not supported under a data-parallel launcher"):
    explain.explain(Ranked(), Data(2))
assert sys.modules["torch"] is None and "ursonet_amd.hip" not in sys.modules and "ursonet_amd.engine" not in sys.modules
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == set(hip.SIDE_SYMBOLS["explain"]) == NAMES and build.SIDE_SOURCES["explain"] == ["explain.hip"]
    for macro in ("COLS", "MAX_MAPS", "D_ORI", "D_LOC", "ORI_KL", "ORI_TV", "ORI_DROP", "ORI_ARGMAX", "LOC_KL", "LOC_TV", "LOC_DROP", "LOC_ARGMAX"):
        v = getattr(X, macro)
        assert re.search(r"#define\s+URSO_OCCL_%s\s+%d\b" % (macro, v), txt), macro
        assert getattr(hip, "OCCL_" + macro) == v
    assert (X.DEC_LOC_EST, X.DEC_Q_EST, X.DEC_COLS) == (hip.DEC_LOC_EST, hip.DEC_Q_EST, hip.DEC_COLS)
    assert X.ORI_KL + 4 == X.LOC_KL and X.LOC_KL + 4 == X.COLS and len(X.MAP_COLUMNS) == X.MAX_MAPS
    # the argument structs are the header's: field order and sizes
    fields = {"urso_occl_fill_args": (hip.OcclFillArgs, ["B", "n", "H", "W", "C", "fill", "src", "rects", "out"], 48),
              "urso_occl_score_args": (hip.OcclScoreArgs, ["B", "n", "row0", "ori_K", "ori_ld", "loc_K", "loc_ld", "dec0", "dec", "ori_z0", "ori_z",
                                                           "loc_z0", "loc_z", "out"], 88),
              "urso_occl_splat_args": (hip.OcclSplatArgs, ["P", "M", "wy0", "wx0", "h", "w", "cols", "ld", "scores", "rects", "out"], 88),
              "urso_heat_overlay_args": (hip.HeatOverlayArgs, ["h", "w", "alpha", "pad", "ld_img", "lo", "scale", "map", "lut", "img"], 64)}
    for struct, (cls, order, size) in fields.items():
        assert [f[0] for f in cls._fields_] == order and C.sizeof(cls) == size, struct
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), txt, re.S).group(1)
        body = re.sub(r"\[\w+\]", "", body)
        declared = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"\b(const|int32_t|int64_t|uint8_t|float|double|void)\b|\*", " ", body))
        assert declared == order, struct
    assert hip.OcclFillArgs.fill.offset == 20 and hip.OcclFillArgs.src.offset == 24 and hip.OcclScoreArgs.dec0.offset == 32
    assert hip.OcclSplatArgs.cols.offset == 24 and hip.OcclSplatArgs.ld.offset == 56 and hip.HeatOverlayArgs.lo.offset == 24


def test_header_is_plain_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "explain_abi.c"
    src.write_text('#include "ursonet_explain.h"\n#include <stddef.h>\ntypedef void (*fn)(void);\n'
                   "fn table[] = { (fn)urso_occl_fill_u8, (fn)urso_occl_score, (fn)urso_occl_splat, (fn)urso_heat_overlay_u8 };\n"
                   "size_t sizes(void) { return sizeof(urso_occl_fill_args) + sizeof(urso_occl_score_args) + sizeof(urso_occl_splat_args) + "
                   "sizeof(urso_heat_overlay_args) + URSO_OCCL_COLS + URSO_OCCL_MAX_MAPS; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "explain_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_validation_without_gpu():
    """Every refusal of the four entry points.  Device pointers are made up and never dereferenced: each call is refused before a HIP
    call, or has n = 0 and launches nothing."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("explain")
    P = [0x1000000 * k for k in range(1, 9)]

    def call(fn, cls, base, kw):
        a = cls()
        for k, v in dict(base, **kw).items():
            if k == "cols":
                for m, c in enumerate(v):
                    a.cols[m] = c
            else:
                setattr(a, k, v)
        return fn(C.byref(a), None)
    N = 8 * 16 * 3
    fill_base = dict(B=4, n=3, H=8, W=16, C=3, src=P[0], rects=P[1], out=P[2])
    score_base = dict(B=4, n=3, row0=0, ori_K=64, ori_ld=64, loc_K=0, loc_ld=0, dec0=P[0], dec=P[1], ori_z0=P[2], ori_z=P[3], out=P[4])
    splat_base = dict(P=5, M=2, wy0=0, wx0=0, h=4, w=6, cols=[1, 0], ld=10, scores=P[0], rects=P[1], out=P[2])
    over_base = dict(h=4, w=6, alpha=128, pad=0, ld_img=18, lo=0.0, scale=1.0, map=P[0], lut=P[1], img=P[2])
    rows = [(dict(n=-1), "0 <= n <= B"), (dict(n=5), "0 <= n <= B"), (dict(B=-1, n=0), "0 <= n <= B")]
    fill_bad = rows + [(dict(src=None), "null pointer"), (dict(rects=None), "null pointer"), (dict(out=None), "null pointer"),
                       (dict(B=65536), "B <= 65535"), (dict(H=0), "need H, W >= 1"), (dict(W=-2), "need H, W >= 1"), (dict(C=0), "need 1 <= C <= 4 (got 0)"),
                       (dict(C=5), "need 1 <= C <= 4 (got 5)"), (dict(H=1 << 15, W=1 << 15, C=2), "H W C must stay below 2^31"),
                       (dict(rects=P[1] + 2), "rects must be 4-byte aligned"), (dict(src=P[2]), "src lies inside out"),
                       (dict(src=P[2] + 4 * N - 1), "src lies inside out"), (dict(src=P[2] - N + 1), "src lies inside out")]
    score_bad = rows + [(dict(row0=-1), "row0 must be >= 0"), (dict(dec0=None), "null pointer"), (dict(dec=None), "null pointer"), (dict(out=None), "null pointer"),
                        (dict(ori_K=-1), "ori_K must be >= 0"), (dict(loc_K=-2), "loc_K must be >= 0"), (dict(ori_z0=None), "ori_K = 64 needs both ori_z0 and ori_z"),
                        (dict(ori_z=None), "needs both"), (dict(loc_K=8, loc_ld=8), "loc_K = 8 needs both loc_z0 and loc_z"), (dict(ori_ld=63), "ori_ld 63 < ori_K 64"),
                        (dict(loc_K=8, loc_ld=7, loc_z0=P[5], loc_z=P[6]), "loc_ld 7 < loc_K 8"), (dict(ori_z0=P[2] + 2), "ori_z0 and ori_z must be 4-byte aligned"),
                        (dict(ori_z=P[3] + 1), "must be 4-byte aligned"), (dict(dec0=P[0] + 4), "must be 8-byte aligned"), (dict(dec=P[1] + 4), "must be 8-byte aligned"),
                        (dict(out=P[4] + 4), "must be 8-byte aligned")]
    splat_bad = [(dict(scores=None), "null pointer"), (dict(rects=None), "null pointer"), (dict(out=None), "null pointer"), (dict(P=-1), "P must be >= 0"),
                 (dict(M=0), "need 1 <= M <= 8 (got 0)"), (dict(M=9), "need 1 <= M <= 8 (got 9)"), (dict(h=0), "need h, w >= 1"), (dict(w=-1), "need h, w >= 1"),
                 (dict(h=1 << 16, w=1 << 15), "h w < 2^31"), (dict(cols=[1, 10]), "column 10 (cols[1]) outside [0, ld = 10)"), (dict(cols=[-1, 0]), "column -1 (cols[0])"),
                 (dict(rects=P[1] + 1), "rects must be 4-byte aligned"), (dict(scores=P[0] + 4), "must be 8-byte aligned"), (dict(out=P[2] + 4), "must be 8-byte aligned")]
    over_bad = [(dict(map=None), "null pointer"), (dict(lut=None), "null pointer"), (dict(img=None), "null pointer"), (dict(h=0), "need h, w >= 1"),
                (dict(w=0), "need h, w >= 1"), (dict(alpha=-1), "need 0 <= alpha <= 256 (got -1)"), (dict(alpha=257), "need 0 <= alpha <= 256 (got 257)"),
                (dict(ld_img=17), "ld_img 17 < 3 w = 18"), (dict(lo=float("nan")), "lo and scale must be finite"), (dict(scale=float("inf")), "lo and scale must be finite"),
                (dict(map=P[0] + 4), "map must be 8-byte aligned")]
    for fn, cls, base, name, cases in ((lib.urso_occl_fill_u8, hip.OcclFillArgs, fill_base, "urso_occl_fill_u8", fill_bad),
                                       (lib.urso_occl_score, hip.OcclScoreArgs, score_base, "urso_occl_score", score_bad),
                                       (lib.urso_occl_splat, hip.OcclSplatArgs, splat_base, "urso_occl_splat", splat_bad),
                                       (lib.urso_heat_overlay_u8, hip.HeatOverlayArgs, over_base, "urso_heat_overlay_u8", over_bad)):
        for kw, msg in cases:
            assert call(fn, cls, base, kw) == -1, (name, kw)
            err = hip.last_error()
            assert err.startswith(name + ":") and msg in err, (kw, err)
        assert fn(None, None) == -1 and name + ": null argument struct" in hip.last_error()
    # n = 0 is valid and launches nothing (so it needs no GPU); the refusals come in front of it
    for fn, cls, base in ((lib.urso_occl_fill_u8, hip.OcclFillArgs, fill_base), (lib.urso_occl_score, hip.OcclScoreArgs, score_base)):
        assert call(fn, cls, base, dict(n=0)) == 0 and call(fn, cls, base, dict(n=0, B=0)) == 0
    assert call(lib.urso_occl_score, hip.OcclScoreArgs, score_base, dict(n=0, row0=-1)) == -1
    assert call(lib.urso_occl_fill_u8, hip.OcclFillArgs, fill_base, dict(n=0, src=P[2] + 4 * N)) == 0          # just behind out
    assert call(lib.urso_occl_fill_u8, hip.OcclFillArgs, fill_base, dict(n=0, src=P[2] - N)) == 0              # just in front of it
    assert call(lib.urso_occl_score, hip.OcclScoreArgs, score_base, dict(n=0, ori_K=0, ori_z0=None, ori_z=None)) == 0      # no head at all
