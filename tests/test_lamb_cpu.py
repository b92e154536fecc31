"""LAMB without a GPU (Config.LAMB, ursonet_amd/lamb.py): the configuration rules, the tick against b**t in float64 under a bound counted
from its roundings, the step over flat buffers (padding, trust 1 where the rule says so, the guard, a wrong wave order failing the bit
comparison), the surface of liburso_opt.so, every host refusal of the three entry points (they run before any launch), and what the GPU
test's layout must hold for its claim: only zero or normal float32 intermediates, adapting tensors on both sides of LAMB_CLIP's min."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lamb_layout as LAY
from libsurface import header_symbols
from ursonet_amd import lamb as B
from ursonet_amd import lars as L
from ursonet_amd.config import Config
from util import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_opt.h")
f32, f64 = np.float32, np.float64
U = 2.0 ** -24                                   # unit roundoff of float32
NAMES = {"urso_lamb_moments", "urso_lamb_trust", "urso_lamb_apply"}


def _cfg(**kw):
    c = Config()
    c.OPTIMIZER = "Adam"
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------ configuration
def test_default_is_off_and_inference_ignores_the_key():
    c = Config()
    assert c.LAMB is None and c.LAMB_EPS == 1e-8 and c.LAMB_CLIP is False
    assert B.validate(c) is None and not B.enabled(c, "training")
    assert B.validate(object()) is None                                      # a config from before the keys: off
    on = _cfg(LAMB=1.0)
    assert B.validate(on) == (1.0, 1e-8, False) and B.enabled(on, "training") and not B.enabled(on, "inference")
    assert B.validate(_cfg(LAMB=np.float64(0.5), LAMB_EPS=0, LAMB_CLIP=True)) == (0.5, 0.0, True)
    assert B.validate(_cfg(LAMB=None), world=8) is None                      # off: nothing to refuse under a launcher
    assert B.validate(_cfg(LAMB=None, OPTIMIZER="SGD", LARS=0.001)) is None
    assert B.adapts is L.adapts and B.summary is L.summary


@pytest.mark.parametrize("bad", [True, False, 1, "1.0", 0.0, -1.0, float("nan"), float("inf"), [1.0]])
def test_bad_trust_coefficients_are_refused(bad):
    with pytest.raises(ValueError, match="LAMB"):
        B.validate(_cfg(LAMB=bad))


@pytest.mark.parametrize("key,bad", [("LAMB_EPS", -1e-8), ("LAMB_EPS", float("nan")), ("LAMB_EPS", float("inf")), ("LAMB_EPS", "1e-8"),
                                     ("LAMB_EPS", True), ("LAMB_EPS", None), ("LAMB_CLIP", 1), ("LAMB_CLIP", 0), ("LAMB_CLIP", None),
                                     ("LAMB_CLIP", "True")])
def test_bad_eps_and_clip_are_refused(key, bad):
    with pytest.raises(ValueError, match=key):
        B.validate(_cfg(LAMB=1.0, **{key: bad}))


def test_sgd_lars_a_launcher_and_the_model_refuse(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="LAMB.*SGD.*LARS"):
        B.validate(_cfg(LAMB=1.0, OPTIMIZER="SGD"))
    with pytest.raises(ValueError, match="LAMB and LARS"):
        B.validate(_cfg(LAMB=1.0, LARS=0.001))
    with pytest.raises(ValueError, match="LAMB and LARS"):
        B.validate(_cfg(LAMB=1.0, LARS=0.001, OPTIMIZER="SGD"))
    with pytest.raises(ValueError, match="LAMB.*data parallelism.*world size 2"):
        B.validate(_cfg(LAMB=1.0), world=2)
    # LARS with Adam keeps raising, with or without this key
    with pytest.raises(ValueError, match="LARS.*LAMB.*not built"):
        L.validate(_cfg(LARS=0.001))
    # the data-parallel wrapper refuses an engine that carries the launches (a stub engine: the refusals come before it touches anything else)
    import types
    from ursonet_amd import dp
    monkeypatch.setattr(dp.dist, "get_world_size", lambda group=None: 2)
    stub = types.SimpleNamespace(ls_state=None, learn_lw=False, ema_state=None, lars_plan=None, lamb_plan=object(), mode="training",
                                 config=_cfg(LAMB=1.0))
    with pytest.raises(ValueError, match="LAMB.*data parallelism.*world size 2"):
        dp.DataParallelEngine(stub, comm_cus=0)
    # at build, through the model: refused before any engine exists (so this needs no GPU)
    from ursonet_amd.net import UrsoNet
    for kw in (dict(LAMB=True), dict(LAMB=1), dict(LAMB=-0.5), dict(LAMB=1.0, LAMB_EPS=-1.0), dict(LAMB=1.0, LAMB_CLIP=1),
               dict(LAMB=1.0, OPTIMIZER="SGD"), dict(LAMB=1.0, LARS=0.001)):
        cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
        cfg.OPTIMIZER = "Adam"
        for k, v in kw.items():
            setattr(cfg, k, v)
        with pytest.raises(ValueError, match="LAMB"):
            UrsoNet("training", cfg, str(tmp_path), build_engine=True)


# ------------------------------------------------------------------ the tick
def test_tick_is_exact_at_one_and_within_its_roundings_of_the_powers():
    """p after t ticks is t - 1 rounded products of float32 numbers (the first, 1 * b, is exact): relative error at most
    (1 + U)^(t - 1) - 1 against b**t in float64 (whose own error, 2^-53 per product, is far below).  kt is then three more operations of
    these p, each rounded once: checked as the same statements."""
    hyper, state = LAY.hyper_state(5.0, t=0)
    assert state.tolist() == [1.0, 1.0, 0.0] and hyper[5] == 0
    b1, b2 = f64(hyper[1]), f64(hyper[2])
    for t in range(1, 51):
        h2, s2 = B.tick32(hyper, state)
        assert h2 is not hyper and s2 is not state and h2.dtype == f32 and s2.dtype == f32
        assert h2[5] == t and np.array_equal(_bits(np.delete(h2, 5)), _bits(np.delete(hyper, 5)))      # t alone moves in hyper
        hyper, state = h2, s2
        for p, b in ((state[0], b1), (state[1], b2)):
            assert abs(f64(p) - b ** t) <= ((1 + U) ** (t - 1) - 1) * b ** t, (t, p, b ** t)
        if t == 1:
            assert state[0] == hyper[1] and state[1] == hyper[2]              # exact
        assert _bits(state[2:3])[0] == _bits(np.array([f32(np.sqrt(f32(f32(1) - state[1])) / f32(f32(1) - state[0]))]))[0]
    # Keras's factor from the same float32 betas: a few 1e-5 apart at t = 1 (1 - b2^t cancels), closing in as t grows
    assert abs(f64(state[2]) - np.sqrt(1 - b2 ** 50) / (1 - b1 ** 50)) < 1e-4


# ------------------------------------------------------------------ the pieces
def test_moments_direction_and_apply_are_the_written_statements():
    rng = np.random.default_rng(3)
    n = 1000
    g, m, w = (rng.standard_normal(n).astype(f32) for _ in range(3))
    v = np.square(rng.standard_normal(n)).astype(f32)
    vhat = (v * rng.uniform(0.5, 2, n)).astype(f32)
    hyper, state = LAY.hyper_state(5.0)
    c = f32(0.37)
    m2, v2, h2 = B.moments32(g, m, v, vhat, hyper, c)
    r = B.direction32(m2, h2, state[2], hyper[3])
    w2 = B.apply32(w, r, hyper[0], f32(0.25))
    for i in range(0, n, 97):                                                # scalar by scalar, each operation rounded once
        gi = f32(g[i] * c)
        mi = f32(f32(hyper[1] * m[i]) + f32(hyper[6] * gi))
        vi = f32(f32(hyper[2] * v[i]) + f32(hyper[7] * f32(gi * gi)))
        hi = max(vhat[i], vi)
        ri = f32(f32(state[2] * mi) / f32(f32(np.sqrt(hi)) + hyper[3]))
        wi = f32(w[i] - f32(f32(hyper[0] * f32(0.25)) * ri))
        assert (m2[i], v2[i], h2[i], r[i], w2[i]) == (mi, vi, hi, ri, wi), i
    assert (h2 > vhat).any() and (h2 == vhat).any()                          # both sides of the max
    # against float64 within the roundings of the statements: m two products and a sum, r three more operations
    m64 = f64(hyper[1]) * m.astype(f64) + f64(hyper[6]) * (g.astype(f64) * f64(c))
    assert np.all(np.abs(m2 - m64) <= 4 * U * (np.abs(f64(hyper[1]) * m) + np.abs(f64(hyper[6]) * g * f64(c))))
    r64 = f64(state[2]) * m2.astype(f64) / (np.sqrt(h2.astype(f64)) + f64(hyper[3]))
    assert np.all(np.abs(r - r64) <= 5 * U * np.abs(r64))


def test_trust_branches():
    eta, eps = 1.0, 1e-8
    assert B.trust32(0.0, 3.0, eta, eps, False) == 1 and B.trust32(3.0, 0.0, eta, eps, False) == 1
    assert B.trust32(0.0, 0.0, eta, eps, True) == 1 and B.trust32(5.0, 3.0, eta, eps, False, adapt=False) == 1
    q = B.trust64(5.0, 3.0, eta, eps, False)
    assert q == f64(eta) * f64(5.0) / (f64(3.0) + f64(eps)) and q.dtype == f64
    t = B.trust32(5.0, 3.0, eta, eps, False)
    assert t.dtype == f32 and t == f32(q) and t > 1
    assert B.trust32(5.0, 3.0, eta, eps, True) == 1                          # LAMB_CLIP: min(q, 1)
    assert B.trust32(3.0, 5.0, eta, eps, True) == B.trust32(3.0, 5.0, eta, eps, False) == f32(B.trust64(3.0, 5.0, eta, eps, False)) < 1
    assert B.trust64(1.0, 1e-30, eta, 0.0, False) > 1e29 and B.trust64(1.0, 1e-30, eta, 1e-8, False) < 1.0001e8


# ------------------------------------------------------------------ the step
TENSORS = [(0, 5, True), (8, 4097, True), (4108, 3, False), (4112, 7, True)]


def _small():
    rng = np.random.default_rng(9)
    n = 4120
    w, g, m = (rng.standard_normal(n).astype(f32) for _ in range(3))
    v = np.square(rng.standard_normal(n)).astype(f32)
    vhat = (v * rng.uniform(0.5, 2, n)).astype(f32)
    for x in (g, m, v, vhat):
        x[4112:4119] = 0                                                     # a frozen layer: zero gradient and moments
    used = np.zeros(n, dtype=bool)
    for o, k, _ in TENSORS:
        used[o:o + k] = True
    return w, g, m, v, vhat, used, f32(np.square(g[used].astype(f64)).sum())


def test_step32_leaves_padding_and_skips_on_a_non_finite_norm():
    w, g, m, v, vhat, used, normsq = _small()
    hyper, state = LAY.hyper_state(5.0)
    w2, m2, v2, h2, hyp2, st2, trust, stat = B.step32(w, g, m, v, vhat, TENSORS, hyper, state, normsq, 1.0, 1e-8, False)
    for new, old in ((w2, w), (m2, m), (v2, v), (h2, vhat)):
        assert new is not old and np.array_equal(_bits(new[~used]), _bits(old[~used]))
    assert hyp2[5] == 4 and st2.tobytes() == B.tick32(hyper, state)[1].tobytes()
    assert trust.dtype == f32 and stat.dtype == f64 and stat.shape == (4, 3)
    assert trust[2] == 1 and stat[2, 2] == 1 and stat[2, 0] > 0 and stat[2, 1] > 0      # not adapting: norms reported, trust 1
    assert trust[3] == 1 and stat[3, 1] == 0 and stat[3, 0] > 0               # zero gradient and moments: r = 0
    assert np.array_equal(_bits(w2[4112:4119]), _bits(w[4112:4119]))          # ... and it does not move
    assert trust[0] != 1 and trust[1] != 1 and trust[0] > 0 and trust[1] > 0
    c = L.clip_factor32(normsq, 5.0)
    assert c < 1                                                             # the clip is active in this case
    for t, (o, k, _a) in enumerate(TENSORS):
        s = slice(o, o + k)
        em, ev, eh = B.moments32(g[s], m[s], v[s], vhat[s], hyper, c)
        r = B.direction32(em, eh, st2[2], hyper[3])
        assert m2[s].tobytes() == em.tobytes() and v2[s].tobytes() == ev.tobytes() and h2[s].tobytes() == eh.tobytes()
        assert w2[s].tobytes() == B.apply32(w[s], r, hyper[0], trust[t]).tobytes()
        assert stat[t, 0] == L.norms64(L.slot_sums32(w[s])) and stat[t, 1] == L.norms64(L.slot_sums32(r))
        assert trust[t] == B.trust32(stat[t, 0], stat[t, 1], 1.0, 1e-8, False, _a)
    # the loss-scaled form: a non-finite norm changes nothing, the state included; a finite one is the plain form
    for bad in (np.inf, np.nan):
        res = B.step32(w, g, m, v, vhat, TENSORS, hyper, state, bad, 1.0, guard=True)
        for new, old in zip(res[:6], (w, m, v, vhat, hyper, state)):
            assert new.tobytes() == old.tobytes()
        assert res[6] is None and res[7] is None
    res = B.step32(w, g, m, v, vhat, TENSORS, hyper, state, normsq, 1.0, guard=True)
    assert res[0].tobytes() == w2.tobytes() and res[6].tobytes() == trust.tobytes()


def test_a_wrong_wave_order_fails_the_bit_comparison():
    right = LAY.reference(1e4, False)[0]
    wrong = LAY.reference(1e4, False, wave_order=(3, 2, 1, 0))[0]
    assert np.allclose(right[7], wrong[7], rtol=1e-6) and right[7].tobytes() != wrong[7].tobytes()      # stat sees the order
    assert (_bits(right[7]) != _bits(wrong[7])).sum() >= 4                   # not one lucky slot
    assert right[6].tobytes() != wrong[6].tobytes() and right[0].tobytes() != wrong[0].tobytes()        # and so do trust and the weights
    assert right[1].tobytes() == wrong[1].tobytes()                          # the moments do not depend on it


# ------------------------------------------------------------------ what the GPU test's layout must hold
@pytest.mark.parametrize("clip", LAY.CLIPS)
def test_the_gpu_layout_holds_only_zero_or_normal_intermediates(clip):
    """So flush-to-zero behaviour is no part of the GPU test's claim: every float32 the kernels store or hold in between, over both
    consecutive steps, is zero or a normal number (and finite)."""
    lay = LAY.layout()
    assert (L.clip_factor32(lay["normsq"], clip) < 1) == (clip == 1e4)
    tiny = np.finfo(f32).tiny
    inter = []
    LAY.reference(clip, False, steps=2, intermediates=inter)
    assert len(inter) == 2 * len(LAY.SIZES) * 19
    for a in inter:
        a = np.asarray(a, dtype=f32)
        assert np.isfinite(a).all() and ((a == 0) | (np.abs(a) >= tiny)).all()
    hyper, state = LAY.hyper_state(clip)
    for x in (hyper, state, B.tick32(hyper, state)[1], B.tick32(*B.tick32(hyper, state))[1]):
        assert np.isfinite(x).all() and ((x == 0) | (np.abs(x) >= tiny)).all()


def test_the_gpu_layout_lies_on_both_sides_of_the_clip_and_has_its_cases():
    lay = LAY.layout()
    for name in LAY.NAMES:                                                   # the sentinel everywhere outside the tensors
        assert (_bits(lay[name][~lay["used"]]) == LAY.SENTINEL).all() and np.isfinite(lay[name][lay["used"]]).all()
    assert (lay["v"][lay["used"]] >= 0).all() and (lay["vhat"][lay["used"]] >= 0).all()
    assert all(o % 4 == 0 for o, _n, _a in lay["tensors"]) and [n for _o, n, _a in lay["tensors"]] == LAY.SIZES
    adapting = [t for t in range(len(LAY.SIZES)) if t not in LAY.PLAIN + (LAY.ZERO_G, LAY.ZERO_W)]
    for clip in LAY.CLIPS:
        (_w, _m, _v, _h, _hy, _st, trust, stat), = LAY.reference(clip, False)
        q = stat[:, 2]
        assert any(q[t] > 1 for t in adapting) and any(q[t] < 1 for t in adapting)          # both sides of LAMB_CLIP's min
        trust_c = LAY.reference(clip, True)[0][6]
        assert all(trust_c[t] == min(trust[t], f32(1)) for t in range(len(q)))
        assert trust[LAY.ZERO_G] == 1 and stat[LAY.ZERO_G, 1] == 0 and stat[LAY.ZERO_G, 0] > 0
        assert trust[LAY.ZERO_W] == 1 and stat[LAY.ZERO_W, 0] == 0 and stat[LAY.ZERO_W, 1] > 0
        for t in LAY.PLAIN:
            assert trust[t] == 1 and stat[t, 2] == 1 and stat[t, 0] > 0 and stat[t, 1] > 0


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == NAMES == set(hip.SIDE_SYMBOLS["opt"]) and build.SIDE_SOURCES["opt"] == ["lamb.hip"]
    assert re.search(r"#define\s+URSO_LAMB_STATE\s+3\b", txt) and len(hip.LAMB_STATE_INIT) == 3 and tuple(hip.LAMB_STATE_INIT) == B.STATE_INIT


def test_header_is_plain_c99(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "opt_abi.c"
    src.write_text('#include "ursonet_opt.h"\n#include <stddef.h>\ntypedef void (*fn)(void);\nfn table[] = {\n' +
                   "".join("    (fn)%s,\n" % n for n in sorted(NAMES)) + "};\nsize_t count(void) { return sizeof(table) / sizeof(table[0]); }\n"
                   "int state_floats(void) { return URSO_LAMB_STATE; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-Wno-pedantic", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "opt_abi.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _i64(vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*vals)


def test_argument_validation_without_gpu():
    """Every refusal of the three launches.  Device pointers are made up and never dereferenced: each call is refused before a launch, or
    has T = 0 / no blocks and launches nothing; the host tables are real."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("opt")
    W, G, M, V, H, TAB, MAP, PART, FIRST, ADAPT, HYP, ST, NSQ, TR, STAT, LS = (0x10000 * k for k in range(1, 17))
    off, n = _i64([0, 8, 4108]), _i64([5, 4097, 3])
    nb = 1 + 2 + 1
    good_m = dict(T=3, off=off, n=n, tab=TAB, map=MAP, nb=nb, w=W, g=G, m=M, v=V, vhat=H, hyper=HYP, state=ST, normsq=NSQ, part=PART, ls=None)
    five = "five different"
    bad_m = [(dict(w=None), "null"), (dict(g=None), "null"), (dict(m=None), "null"), (dict(v=None), "null"), (dict(vhat=None), "null"),
             (dict(hyper=None), "null"), (dict(state=None), "null"), (dict(normsq=None), "null"), (dict(tab=None), "null"),
             (dict(map=None), "null"), (dict(part=None), "null"), (dict(off=None), "null"), (dict(n=None), "null"),
             (dict(T=-1), "T must be >= 0"), (dict(off=_i64([0, 6, 4108])), "multiple of 4"), (dict(off=_i64([0, -4, 4108])), "multiple of 4"),
             (dict(n=_i64([5, -1, 3]), nb=2), "negative size"),
             (dict(w=W + 4), "16-byte aligned"), (dict(g=G + 8), "16-byte aligned"), (dict(m=M + 4), "16-byte aligned"),
             (dict(v=V + 12), "16-byte aligned"), (dict(vhat=H + 4), "16-byte aligned"), (dict(tab=TAB + 4), "8-byte aligned"),
             (dict(part=PART + 4), "8-byte aligned"), (dict(map=MAP + 2), "4-byte aligned"), (dict(state=ST + 2), "4-byte aligned"),
             (dict(hyper=HYP + 1), "4-byte aligned"), (dict(ls=LS + 2), "4-byte aligned"),
             (dict(off=_i64([0, 4, 4108])), "overlap"), (dict(off=_i64([4108, 8, 0]), n=_i64([3, 4097, 12])), "overlap"),
             (dict(off=_i64([0, 8, 4104])), "overlap"), (dict(nb=nb - 1), "nblocks"), (dict(nb=nb + 1), "nblocks"), (dict(nb=0), "nblocks"),
             (dict(g=W), five), (dict(m=W), five), (dict(v=G), five), (dict(vhat=M), five), (dict(vhat=V), five), (dict(m=G), five)]

    def call(fn, good, kw):
        a = dict(good, **kw)
        return getattr(lib, fn)(*[a[k] for k in good], None)
    for kw, msg in bad_m:
        assert call("urso_lamb_moments", good_m, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_lamb_moments:") and msg in err, (kw, err)
    good_a = dict(T=3, off=off, n=n, tab=TAB, map=MAP, nb=nb, w=W, m=M, vhat=H, trust=TR, hyper=HYP, state=ST, normsq=NSQ, ls=None)
    bad_a = [(dict(w=None), "null"), (dict(m=None), "null"), (dict(vhat=None), "null"), (dict(trust=None), "null"), (dict(hyper=None), "null"),
             (dict(state=None), "null"), (dict(normsq=None), "null"), (dict(tab=None), "null"), (dict(map=None), "null"),
             (dict(off=None), "null"), (dict(n=None), "null"), (dict(T=-3), "T must be >= 0"), (dict(off=_i64([0, 10, 4108])), "multiple of 4"),
             (dict(w=W + 4), "16-byte aligned"), (dict(m=M + 4), "16-byte aligned"), (dict(vhat=H + 12), "16-byte aligned"),
             (dict(tab=TAB + 4), "8-byte aligned"), (dict(trust=TR + 1), "4-byte aligned"), (dict(ls=LS + 2), "4-byte aligned"),
             (dict(state=ST + 2), "4-byte aligned"), (dict(off=_i64([0, 4, 4108])), "overlap"), (dict(nb=nb + 2), "nblocks"),
             (dict(m=W), "three different"), (dict(vhat=W), "three different"), (dict(vhat=M), "three different")]
    for kw, msg in bad_a:
        assert call("urso_lamb_apply", good_a, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_lamb_apply:") and msg in err, (kw, err)
    good_t = dict(T=3, first=FIRST, adapt=ADAPT, nb=nb, part=PART, normsq=NSQ, eta=1.0, eps=1e-8, clip=0, trust=TR, stat=STAT, ls=None)
    bad_t = [(dict(first=None), "null"), (dict(adapt=None), "null"), (dict(part=None), "null"), (dict(normsq=None), "null"),
             (dict(trust=None), "null"), (dict(stat=None), "null"), (dict(T=-1), "T must be >= 0"),
             (dict(nb=-1), "nblocks"), (dict(eta=0.0), "eta"), (dict(eta=-1.0), "eta"), (dict(eta=float("nan")), "eta"),
             (dict(eta=float("inf")), "eta"), (dict(eps=-1e-9), "eps"), (dict(eps=float("nan")), "eps"), (dict(clip=2), "clip_mode"),
             (dict(clip=-1), "clip_mode"), (dict(part=PART + 4), "8-byte aligned"), (dict(stat=STAT + 4), "8-byte aligned"),
             (dict(trust=TR + 2), "4-byte aligned"), (dict(first=FIRST + 1), "4-byte aligned")]
    for kw, msg in bad_t:
        assert call("urso_lamb_trust", good_t, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_lamb_trust:") and msg in err, (kw, err)
    # T = 0 is valid and launches nothing (so it needs no GPU); so do tensors that are all empty
    assert lib.urso_lamb_moments(0, None, None, None, None, 0, W, G, M, V, H, HYP, ST, NSQ, None, None, None) == 0
    assert lib.urso_lamb_trust(0, None, None, 0, None, NSQ, 1.0, 0.0, 1, None, None, None, None) == 0
    assert lib.urso_lamb_apply(0, None, None, None, None, 0, W, M, H, None, HYP, ST, NSQ, None, None) == 0
    assert lib.urso_lamb_moments(2, _i64([0, 0]), _i64([0, 0]), None, None, 0, W, G, M, V, H, HYP, ST, NSQ, None, None, None) == 0
    assert lib.urso_lamb_apply(2, _i64([0, 0]), _i64([0, 0]), None, None, 0, W, M, H, None, HYP, ST, NSQ, None, None) == 0


def test_module_imports_neither_torch_nor_the_library():
    code = "import sys; import ursonet_amd.lamb; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
