"""SAM without a GPU (Config.SAM): the keys and their refusals, the NumPy rule of ursonet_amd/sam.py against float64
within bounds counted from its roundings, the cases that move nothing, the bit-copy way back, the state's arithmetic (the ascent's record
and the settlement of a skipped step), the surface of liburso_train.so (header, bindings and library agree; no name of the other three
libraries), and every refusal of the entry points with made-up pointers that are never dereferenced."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

from libsurface import header_symbols
from ursonet_amd import sam as S
from ursonet_amd.config import Config
from util import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_train.h")

U = 2.0 ** -24                                   # unit roundoff of float32
SAM_NAMES = {"urso_sam_ascend", "urso_sam_descend", "urso_sam_settle"}


def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.asarray(a).shape == np.asarray(b).shape and np.array_equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ configuration
def test_default_is_off_and_inference_ignores_the_key():
    c = Config()
    assert c.SAM is None and c.SAM_EPS == 1e-12
    assert S.validate(c) is None and not S.enabled(c, "training")
    assert S.validate(object()) is None                                      # a config from before the keys: off
    on = _cfg(SAM=0.05)
    assert S.validate(on) == (0.05, 1e-12) and S.enabled(on, "training") and not S.enabled(on, "inference")
    assert S.validate(_cfg(SAM=np.float64(0.5), SAM_EPS=0)) == (0.5, 0.0)
    assert S.validate(_cfg(SAM=np.float32(0.25), SAM_EPS=np.float32(0.5))) == (0.25, 0.5)
    assert S.validate(_cfg(SAM=None), world=8) is None                       # off: nothing to refuse under a launcher
    for opt in ("SGD", "Adam"):                                              # either optimizer, and the layer-wise rules
        assert S.validate(_cfg(SAM=0.05, OPTIMIZER=opt)) == (0.05, 1e-12)
    assert S.validate(_cfg(SAM=0.05, OPTIMIZER="SGD", LARS=0.001)) and S.validate(_cfg(SAM=0.05, OPTIMIZER="Adam", LAMB=1.0))
    assert S.STATE_LEN == 8 and len(S.STATE_INIT) == 8 and not any(S.STATE_INIT)
    assert (S.RHO, S.EPS, S.NORMSQ, S.SCALE, S.APPLIED, S.APPLIED_TOTAL, S.PENDING) == (0, 1, 2, 3, 4, 5, 6)
    assert S.initial_state(0.05, 1e-12) == (0.05, 1e-12, 0, 0, 0, 0, 0, 0)


@pytest.mark.parametrize("bad", [True, False, 1, 0, "0.05", 0.0, -0.05, float("nan"), float("inf"), -float("inf"), [0.05], np.True_])
def test_bad_rho_is_refused(bad):
    with pytest.raises(ValueError, match="SAM must be"):
        S.validate(_cfg(SAM=bad))
    with pytest.raises(ValueError, match="SAM"):
        S.enabled(_cfg(SAM=bad), "training")


@pytest.mark.parametrize("bad", [-1e-12, float("nan"), float("inf"), "1e-12", True, None, [0.0]])
def test_bad_eps_is_refused_on_or_off(bad):
    for rho in (0.05, None):
        with pytest.raises(ValueError, match="SAM_EPS"):
            S.validate(_cfg(SAM=rho, SAM_EPS=bad))


def test_a_launcher_the_wrapper_and_the_model_refuse(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="SAM.*data parallelism.*world size 2"):
        S.validate(_cfg(SAM=0.05), world=2)
    # the data-parallel wrapper refuses an engine that carries the state (a stub engine: the refusals come before it touches anything else)
    from ursonet_amd import dp
    monkeypatch.setattr(dp.dist, "get_world_size", lambda group=None: 2)
    stub = types.SimpleNamespace(ls_state=None, learn_lw=False, ema_state=None, lars_plan=None, lamb_plan=None, sam_state=object(),
                                 mode="training", config=_cfg(SAM=0.05))
    with pytest.raises(ValueError, match="SAM.*data parallelism.*world size 2"):
        dp.DataParallelEngine(stub, comm_cus=0)
    # at build, through the model: refused before any engine exists (so this needs no GPU)
    from ursonet_amd.net import UrsoNet
    for kw in (dict(SAM=True), dict(SAM=1), dict(SAM=-0.5), dict(SAM="0.05"), dict(SAM=float("nan")), dict(SAM=0.05, SAM_EPS=-1.0),
               dict(SAM=None, SAM_EPS="x")):
        cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
        for k, v in kw.items():
            setattr(cfg, k, v)
        with pytest.raises(ValueError, match="SAM"):
            UrsoNet("training", cfg, str(tmp_path), build_engine=True)
    # ... and under a launcher (world size 2 in the environment), with good keys
    cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
    cfg.SAM = 0.05
    monkeypatch.setattr(dp, "launcher_world", lambda: (0, 0, 2))
    with pytest.raises(ValueError, match="SAM.*data parallelism.*world size 2"):
        UrsoNet("training", cfg, str(tmp_path), build_engine=True)


# ------------------------------------------------------------------ the rule
def _case(n=4099, seed=5, gscale=1.0):
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n).astype(np.float32)
    g = (rng.standard_normal(n) * gscale).astype(np.float32)
    g[::7] = 0.0
    normsq = np.float32(np.sum(g.astype(np.float64) ** 2))                   # |g|^2 rounded once
    return w, g, normsq


@pytest.mark.parametrize("rho,eps,gscale", [(0.05, 1e-12, 1.0), (0.05, 1e-12, 1e-3), (2.0, 0.0, 30.0), (0.5, 0.25, 1.0)])
def test_ascend32_is_within_its_roundings_of_float64(rho, eps, gscale):
    """The device holds rho and eps as float32, so the float64 reference takes those values.  With s* = rho / (sqrt(N) + eps) exact:
    sqrtf, the sum with eps (both terms >= 0) and the division each add a relative u, so |s - s*| <= 3u s* to first order; the product s g
    adds one more: |e - s* g| <= 4u |s* g|; the last sum adds u |w + e|.  Bound: 4u |s* g| + u |w + s* g|, with 1 % for the second-order
    terms, plus half a subnormal spacing."""
    w, g, normsq = _case(gscale=gscale)
    w1, w0, s, applied = S.ascend32(w, g, normsq, rho, eps)
    assert applied and w1.dtype == w0.dtype == np.float32 and _same_bits(w0, w)
    r32, e32 = np.float64(np.float32(rho)), np.float64(np.float32(eps))
    s64 = r32 / (np.sqrt(np.float64(normsq)) + e32)
    assert abs(np.float64(s) - s64) <= 3.03 * U * s64
    sg = s64 * g.astype(np.float64)
    exact = w.astype(np.float64) + sg
    bound = 1.01 * (4 * U * np.abs(sg) + U * np.abs(exact)) + 2.0 ** -150
    assert (np.abs(w1.astype(np.float64) - exact) <= bound).all()
    assert _same_bits(w1[::7], (w[::7] + np.float32(0.0)).astype(np.float32))    # g = 0: the value does not move
    assert np.array_equal(w1[::7], w[::7]) and not np.array_equal(w1, w)
    # the length of the move against rho |g| / (|g| + eps), |g| the exact norm of g: N is |g|^2 rounded once (u / 2 on the root, once in s
    # and once in the target's own |g|), s carries 3u, each product u (so their norm u): 5u in all, with 1 % for the second order
    e = (s * g).astype(np.float32).astype(np.float64)
    gn = np.sqrt(np.sum(g.astype(np.float64) ** 2))
    target = r32 * gn / (gn + e32)
    assert abs(np.sqrt(np.sum(e ** 2)) - target) <= 1.01 * 5 * U * target


def test_scale32_is_three_rounded_operations():
    for normsq, rho, eps in ((np.float32(7.3), 0.05, 1e-12), (np.float32(1e-20), 0.05, 1e-12), (np.float32(3e30), 1.5, 0.5),
                             (np.float32(2.0 ** -149), 0.05, 0.0)):
        s, applied = S.scale32(normsq, rho, eps)
        root = np.float32(np.sqrt(np.float32(normsq)))
        den = np.float32(root + np.float32(eps))
        assert applied and type(s) is np.float32 and _same_bits(s, np.float32(np.float32(rho) / den)) and np.isfinite(s)


@pytest.mark.parametrize("normsq", [0.0, -0.0, float("inf"), float("nan"), -1.0])
def test_a_zero_or_non_finite_norm_moves_nothing(normsq):
    w, g, _ = _case(n=133)
    w[3], w[4] = -0.0, np.float32(2.0 ** -140)
    w1, w0, s, applied = S.ascend32(w, g, np.float32(normsq), 0.05, 1e-12)
    assert not applied and s == 0 and _same_bits(s, np.float32(0.0)) and _same_bits(w1, w) and _same_bits(w0, w)
    assert S.scale32(np.float32(normsq), 0.05, 0.0) == (0.0, False)
    st = S.ascend_state32(S.initial_state(0.05, 1e-12)[:2] + (normsq, 9.0, 1.0, 4.0, 1.0, 0.0))
    assert st[S.SCALE] == 0 and st[S.APPLIED] == 0 and st[S.APPLIED_TOTAL] == 4 and st[S.PENDING] == 1


def test_descend_of_ascend_is_the_input_bit_for_bit():
    w, g, normsq = _case(n=257)
    w[:6] = np.array([-0.0, 0.0, 2.0 ** -149, -2.0 ** -140, 2.0 ** -126, -3.0e38], dtype=np.float32)
    g[:6] = np.array([0.0, -0.0, 1.0, -1.0, 0.0, -3.0e38], dtype=np.float32)
    nan = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]        # a NaN with a payload is moved like any other bits
    w[6] = nan
    w1, w0, s, applied = S.ascend32(w, g, normsq, 0.05, 1e-12)
    assert applied and _same_bits(w0, w)
    assert _bits(w1)[0] == 0 and _bits(w)[0] == 0x80000000                   # -0.0 + 0.0 = +0.0 while perturbed ...
    back = S.descend32(w1, w0)
    assert _same_bits(back, w) and back is not w0                            # ... and its bits are back afterwards
    assert not _same_bits(w1, w)


def test_state_records_the_ascent_and_a_skipped_step_is_settled():
    st = np.array(S.initial_state(0.05, 1e-12), dtype=np.float32)
    st[S.NORMSQ] = 4.0
    a = S.ascend_state32(st)
    s, _ = S.scale32(np.float32(4.0), 0.05, 1e-12)
    assert _same_bits(a[S.SCALE], s) and a[S.APPLIED] == 1 and a[S.APPLIED_TOTAL] == 1 and a[S.PENDING] == 1
    assert _same_bits(a[:3], st[:3]) and a[7] == 0 and _same_bits(st[3:], np.zeros(5, np.float32))       # a new array; rho, eps, normsq are only read
    b = S.ascend_state32(a)                                                  # a second micro-step
    assert b[S.APPLIED_TOTAL] == 2 and b[S.PENDING] == 2
    for nsq in (float("inf"), float("nan")):                                # the optimizer skips: both ascents leave the count
        c = S.settle32(b, nsq)
        assert c[S.APPLIED_TOTAL] == 0 and c[S.PENDING] == 0 and _same_bits(c[:5], b[:5])
    c = S.settle32(b, 3.0)                                                   # the step counts
    assert c[S.APPLIED_TOTAL] == 2 and c[S.PENDING] == 0
    c = S.settle32(b, float("inf"), guard=False)
    assert c[S.APPLIED_TOTAL] == 2 and c[S.PENDING] == 0


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    """The three agree with each other and hold the SAM names; the set is not pinned to them: the next training feature goes here."""
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == set(hip.SIDE_SYMBOLS["train"]) and SAM_NAMES <= names and "sam.hip" in build.SIDE_SOURCES["train"]
    assert re.search(r"#define\s+URSO_SAM_STATE\s+8\b", txt) and hip.SAM_STATE == S.STATE_LEN == 8
    for field in ("RHO", "EPS", "NORMSQ", "SCALE", "APPLIED", "APPLIED_TOTAL", "PENDING"):
        assert re.search(r"#define\s+URSO_SAM_%s\s+%d\b" % (field, getattr(S, field)), txt), field


def test_header_is_plain_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    names, _ = header_symbols(HEADER)
    src = tmp_path / "train_abi.c"
    src.write_text('#include "ursonet_train.h"\n#include <stddef.h>\ntypedef void (*fn)(void);\nfn table[] = {\n' +
                   "".join("    (fn)%s,\n" % n for n in sorted(names)) + "};\nsize_t count(void) { return sizeof(table) / sizeof(table[0]); }\n"
                   "int state_floats(void) { return URSO_SAM_STATE + URSO_SAM_PENDING; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "train_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_argument_validation_without_gpu():
    """Every refusal of the entry points.  Device pointers are made up and never dereferenced: each call is refused before a launch, or
    has n = 0 and launches nothing."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("train")
    W, G, W0, ST, NSQ = (0x10000 * k for k in range(1, 6))
    good_a = dict(n=1000, w=W, g=G, w0=W0, state=ST)
    three = "three buffers"
    bad_a = [(dict(w=None), "null"), (dict(g=None), "null"), (dict(w0=None), "null"), (dict(state=None), "null"),
             (dict(n=-1), "n must be >= 0"), (dict(n=-2 ** 40), "n must be >= 0"),
             (dict(w=W + 2), "4-byte aligned"), (dict(g=G + 1), "4-byte aligned"), (dict(w0=W0 + 3), "4-byte aligned"),
             (dict(state=ST + 2), "4-byte aligned"),
             (dict(g=W), three), (dict(w0=W), three), (dict(w0=G), three), (dict(g=W, w0=W), three)]

    def call(fn, good, kw):
        a = dict(good, **kw)
        return getattr(lib, fn)(*[a[k] for k in good], None)
    for kw, msg in bad_a:
        assert call("urso_sam_ascend", good_a, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_sam_ascend:") and msg in err, (kw, err)
    good_d = dict(n=1000, w=W, w0=W0)
    bad_d = [(dict(w=None), "null"), (dict(w0=None), "null"), (dict(n=-1), "n must be >= 0"), (dict(w=W + 2), "4-byte aligned"),
             (dict(w0=W0 + 1), "4-byte aligned"), (dict(w0=W), "same buffer")]
    for kw, msg in bad_d:
        assert call("urso_sam_descend", good_d, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_sam_descend:") and msg in err, (kw, err)
    good_s = dict(state=ST, normsq=NSQ, guard=1)
    bad_s = [(dict(state=None), "null"), (dict(normsq=None), "null"), (dict(state=ST + 2), "4-byte aligned"),
             (dict(normsq=NSQ + 1), "4-byte aligned"), (dict(guard=2), "guard"), (dict(guard=-1), "guard")]
    for kw, msg in bad_s:
        assert call("urso_sam_settle", good_s, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_sam_settle:") and msg in err, (kw, err)
    # n = 0 is valid and launches nothing (so it needs no GPU), at any alignment of the three
    assert lib.urso_sam_ascend(0, W, G, W0, ST, None) == 0 and lib.urso_sam_ascend(0, W + 4, G + 8, W0 + 12, ST, None) == 0
    assert lib.urso_sam_descend(0, W, W0, None) == 0 and lib.urso_sam_descend(0, W + 4, W0, None) == 0
    # the refusals come in front of n == 0
    assert lib.urso_sam_ascend(0, W, W, W0, ST, None) == -1 and lib.urso_sam_descend(0, W, W, None) == -1


def test_module_imports_neither_torch_nor_the_library():
    code = "import sys; import ursonet_amd.sam; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
