"""Layer-wise adaptive rate scaling without a GPU (Config.LARS, ursonet_amd/lars.py): the configuration rules, the documented reduction
order against a plain float64 sum of squares under a bound counted from its operations, the trust ratio's branches, the update against
float64 within its roundings, a wrong order failing the bit comparison, the host planning and every refusal of the five entry points (they
run before any launch)."""
import ctypes
import os
import re

import numpy as np
import pytest

from ursonet_amd import lars as L
from ursonet_amd.config import Config
from util import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
U = 2.0 ** -24                                   # unit roundoff of float32
U64 = 2.0 ** -53
NAMES = {"urso_lars_blocks", "urso_lars_plan", "urso_lars_norms", "urso_lars_trust", "urso_lars_sgd"}


def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if np.asarray(a).dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------ configuration
def test_default_is_off_and_inference_ignores_the_key():
    c = Config()
    assert c.LARS is None and c.LARS_EPS == 1e-8 and c.LARS_CLIP is False
    assert L.validate(c) is None and not L.enabled(c, "training")
    assert L.validate(object()) is None                                      # a config from before the keys: off
    on = _cfg(LARS=0.001)
    assert L.validate(on) == (0.001, 1e-8, False) and L.enabled(on, "training") and not L.enabled(on, "inference")
    assert L.validate(_cfg(LARS=np.float64(0.02), LARS_EPS=0, LARS_CLIP=True)) == (0.02, 0.0, True)
    assert L.validate(_cfg(LARS=None), world=8) is None                      # off: nothing to refuse under a launcher
    assert L.validate(_cfg(LARS=None, OPTIMIZER="Adam")) is None


@pytest.mark.parametrize("bad", [True, False, 1, "0.001", 0.0, -0.001, float("nan"), float("inf"), [0.001]])
def test_bad_trust_coefficients_are_refused(bad):
    with pytest.raises(ValueError, match="LARS"):
        L.validate(_cfg(LARS=bad))


@pytest.mark.parametrize("key,bad", [("LARS_EPS", -1e-8), ("LARS_EPS", float("nan")), ("LARS_EPS", float("inf")), ("LARS_EPS", "1e-8"),
                                     ("LARS_EPS", True), ("LARS_EPS", None), ("LARS_CLIP", 1), ("LARS_CLIP", 0), ("LARS_CLIP", None),
                                     ("LARS_CLIP", "True")])
def test_bad_eps_and_clip_are_refused(key, bad):
    with pytest.raises(ValueError, match=key):
        L.validate(_cfg(LARS=0.001, **{key: bad}))


def test_adam_a_launcher_and_the_model_refuse(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="LARS.*LAMB.*not built"):
        L.validate(_cfg(LARS=0.001, OPTIMIZER="Adam"))
    with pytest.raises(ValueError, match="LARS.*data parallelism.*world size 2"):
        L.validate(_cfg(LARS=0.001), world=2)
    # the data-parallel wrapper refuses an engine that carries the launches (a stub engine: the refusals come before it touches anything else)
    import types
    from ursonet_amd import dp
    monkeypatch.setattr(dp.dist, "get_world_size", lambda group=None: 2)
    stub = types.SimpleNamespace(ls_state=None, learn_lw=False, ema_state=None, lars_plan=object(), mode="training", config=_cfg(LARS=0.001))
    with pytest.raises(ValueError, match="LARS.*data parallelism.*world size 2"):
        dp.DataParallelEngine(stub, comm_cus=0)
    # at build, through the model: refused before any engine exists (so this needs no GPU)
    from ursonet_amd.net import UrsoNet
    for kw in (dict(LARS=True), dict(LARS=1), dict(LARS=-0.5), dict(LARS=0.001, LARS_EPS=-1.0), dict(LARS=0.001, LARS_CLIP=1),
               dict(LARS=0.001, OPTIMIZER="Adam")):
        cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
        for k, v in kw.items():
            setattr(cfg, k, v)
        with pytest.raises(ValueError, match="LARS"):
            UrsoNet("training", cfg, str(tmp_path), build_engine=True)


def test_which_tensors_adapt():
    assert L.adapts((7, 7, 3, 64)) and L.adapts((1024, 13824)) and L.adapts((1, 1))
    assert not L.adapts((64,)) and not L.adapts(()) and not L.adapts((1,))


# ------------------------------------------------------------------ the sums
def test_chunks():
    assert L.CHUNK == 4096 and L.THREADS == 256 and L.GROUPS == 4
    assert [L.chunks(n) for n in (0, 1, 4095, 4096, 4097, 8192, 8193, 2 ** 33)] == [0, 1, 1, 1, 2, 2, 3, 2 ** 21]
    with pytest.raises(ValueError):
        L.chunks(-1)


def _data(kind, n):
    rng = np.random.default_rng(n)
    if kind == "normal":
        return rng.standard_normal(n).astype(f32)
    if kind == "decades":                                                    # magnitudes over six decades
        return (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
    return np.full(n, f32(1.1), dtype=f32)                                   # every square rounds the same way, every partial sum grows: the worst case


@pytest.mark.parametrize("kind", ["normal", "decades", "constant"])
@pytest.mark.parametrize("n", [1, 3, 5, 255, 4096, 4097, 3 * 4096 + 5, 100003])
def test_slot_sums_and_norms_against_a_plain_float64_sum(kind, n):
    """The bound, counted from the operations.  All terms are >= 0, so every rounding is a relative error of at most U on a partial sum
    that is at most the final one.  A square is rounded once (1) and then passes through at most 16 additions of its thread, 6 of the
    shuffle and 4 of the wave sums: 27 roundings, relative (1 + U)^27 - 1 of the slot.  The float64 additions of the slots add
    chunks * 2^-53, the square root halves the relative error (to first order; the bound below keeps the full one for the sum and
    uses sqrt's monotonicity for the norm) and is rounded once in float64."""
    x = _data(kind, n)
    slots = L.slot_sums32(x, n)
    assert slots.dtype == f32 and slots.shape == (L.chunks(n),)
    exact = np.square(x.astype(f64))                                          # exact: 48 bits
    rel = (1 + U) ** 27 - 1
    for k in range(L.chunks(n)):
        ref = exact[k * L.CHUNK:(k + 1) * L.CHUNK].sum()
        assert abs(f64(slots[k]) - ref) <= rel * ref + 4096 * U64 * ref, (k, slots[k], ref)
    total = exact.sum()
    rel_t = rel + (L.chunks(n) + n) * U64                                    # + the float64 additions of the slots and of this reference
    nrm = L.norms64(slots)
    assert nrm.dtype == f64
    lo, hi = np.sqrt(total * (1 - rel_t)) * (1 - 2 * U64), np.sqrt(total * (1 + rel_t)) * (1 + 2 * U64)
    assert lo <= nrm <= hi, (nrm, np.sqrt(total))
    assert L.slot_sums32(np.concatenate([x, f32([7.0, 7.0])]), n).tobytes() == slots.tobytes()          # elements past n contribute nothing


def test_the_order_is_the_documented_one():
    """An independent restatement with explicit loops over one chunk: thread t owns groups t, 256 + t, 512 + t, 768 + t."""
    x = _data("decades", 4096 + 1000)
    got = L.slot_sums32(x)
    for k, n in ((0, 4096), (1, 1000)):
        chunk = np.zeros(4096, dtype=f32)
        chunk[:n] = x[k * 4096:k * 4096 + n]
        lanes = np.zeros(256, dtype=f32)
        for t in range(256):
            s = f32(0.0)
            for j in range(4):
                for e in range(4):
                    v = chunk[4 * (j * 256 + t) + e]
                    s = f32(s + f32(v * v))
            lanes[t] = s
        waves = []
        for wv in range(4):
            v = lanes[64 * wv:64 * wv + 64].copy()
            for o in (32, 16, 8, 4, 2, 1):
                v = np.array([f32(v[i] + v[i ^ o]) for i in range(64)], dtype=f32)
            assert len(set(v.tobytes()[4 * i:4 * i + 4] for i in range(64))) == 1        # every lane holds the wave's sum
            waves.append(v[0])
        r = f32(0.0)
        for wv in range(4):
            r = f32(r + waves[wv])
        assert _bits(got[k:k + 1])[0] == _bits(np.array([r], dtype=f32))[0]


def test_a_wrong_order_fails_the_bit_comparison():
    x = _data("decades", 64 * 4096)
    right = L.slot_sums32(x)
    wrong = L.slot_sums32(x, wave_order=(3, 2, 1, 0))
    assert np.allclose(right, wrong, rtol=1e-5) and right.tobytes() != wrong.tobytes()
    assert (_bits(right) != _bits(wrong)).sum() >= 4                         # not one lucky chunk: the comparison sees the order
    # the float64 sum of a tensor's slots runs in index order from 0.0
    slots = L.slot_sums32(_data("decades", 200 * 4096))
    s64 = f64(0)
    for a in slots:
        s64 = s64 + f64(a)
    assert L.norms64(slots) == np.sqrt(s64)


# ------------------------------------------------------------------ trust
def test_trust_branches():
    eta, eps, lr = 0.001, 1e-8, f32(0.01)
    one = f32(1.0)
    # zero norms, and tensors that do not adapt: trust 1
    assert L.trust32(0.0, 3.0, eta, eps, False, lr, one) == 1 and L.trust32(3.0, 0.0, eta, eps, False, lr, one) == 1
    assert L.trust32(0.0, 0.0, eta, eps, True, lr, one) == 1 and L.trust32(5.0, 3.0, eta, eps, False, lr, one, adapt=False) == 1
    # the plain ratio, c = 1: float64 arithmetic, rounded once
    q = L.trust64(5.0, 3.0, eta, eps, False, lr, one)
    assert q == f64(eta) * f64(5.0) / (f64(1.0) * f64(3.0) + f64(eps)) and q.dtype == f64
    t = L.trust32(5.0, 3.0, eta, eps, False, lr, one)
    assert t.dtype == f32 and t == f32(q) and abs(f64(t) - 0.001 * 5 / 3) < 1e-9
    # c < 1: the clipped gradient is what the step applies, so its norm is what the ratio sees
    c = L.clip_factor32(f32(400.0), f32(5.0))
    assert c == f32(f32(5.0) / f32(20.0)) and L.clip_factor32(f32(16.0), f32(5.0)) == 1 and L.clip_factor32(f32(400.0), f32(0.0)) == 1
    assert L.clip_factor32(f32(25.0), f32(5.0)) == 1                         # norm >= clip: clip / norm, which is 1 here
    qc = L.trust64(5.0, 3.0, eta, eps, False, lr, c)
    assert qc == f64(eta) * 5.0 / (f64(c) * 3.0 + eps) and qc > 3.9 * q
    # LARS_CLIP: min(q / lr, 1), lr promoted from float32
    assert L.trust32(5.0, 3.0, eta, eps, True, lr, one) == f32(q / f64(lr))
    assert L.trust32(500.0, 3.0, eta, eps, True, lr, one) == 1                # q / lr = 16.7: clipped to the global rate
    assert L.trust32(500.0, 3.0, eta, eps, False, lr, one) == f32(L.trust64(500.0, 3.0, eta, eps, False, lr, one)) > 0.16
    # eps = 0 is legal, and eps keeps a tiny gradient from blowing the ratio up
    assert L.trust64(1.0, 1e-30, eta, 0.0, False, lr, one) > 1e26 and L.trust64(1.0, 1e-30, eta, 1e-8, False, lr, one) < 1.0001e5


def test_update_is_within_its_roundings_of_float64():
    rng = np.random.default_rng(5)
    n = 20000
    w, g, v = (rng.standard_normal(n).astype(f32) for _ in range(3))
    lr, mom, c, trust = f32(0.013), f32(0.9), f32(0.37), f32(0.0021)
    w2, v2 = L.update32(w, g, v, lr, mom, c, trust)
    assert w2.dtype == f32 and v2.dtype == f32 and w2 is not w and v2 is not v
    step = f32(f32(lr * c) * trust)                                          # two float32 products, in this order
    a, b = f64(mom) * v.astype(f64), f64(step) * g.astype(f64)               # exact in float64 (24 x 24 bits)
    v64 = a - b
    # two products and one subtraction, each within U of its exact result
    bound_v = U * (np.abs(a) + np.abs(b)) + U * (np.abs(v64) + U * (np.abs(a) + np.abs(b)))
    assert np.all(np.abs(v2.astype(f64) - v64) <= bound_v)
    assert np.all(np.abs(w2.astype(f64) - (w.astype(f64) + v2.astype(f64))) <= U * np.abs(w.astype(f64) + v2.astype(f64)))   # one addition
    # trust 1 and c = 1 is the plain SGD update, bit for bit
    w3, v3 = L.update32(w, g, v, lr, mom, f32(1), f32(1))
    vp = (mom * v - lr * g).astype(f32)
    assert v3.tobytes() == vp.tobytes() and w3.tobytes() == (w + vp).astype(f32).tobytes()


def test_step32_leaves_padding_and_skips_on_a_non_finite_norm():
    rng = np.random.default_rng(9)
    tensors = [(0, 5, True), (8, 4097, True), (4108, 3, False), (4112, 7, True)]
    n = 4120
    w, g, v = (rng.standard_normal(n).astype(f32) for _ in range(3))
    g[4112:4119] = 0                                                         # a frozen layer: trust 1, and v only decays
    used = np.zeros(n, dtype=bool)
    for o, m, _ in tensors:
        used[o:o + m] = True
    normsq = f32(np.square(g[used].astype(f64)).sum())
    w2, v2, trust, stat = L.step32(w, g, v, tensors, (0.01, 0.9, 5.0), normsq, 0.001)
    assert np.array_equal(_bits(w2[~used]), _bits(w[~used])) and np.array_equal(_bits(v2[~used]), _bits(v[~used]))
    assert trust.dtype == f32 and stat.dtype == f64 and stat.shape == (4, 3)
    assert trust[2] == 1 and stat[2, 2] == 1 and stat[2, 0] > 0 and stat[2, 1] > 0      # not adapting: norms reported, trust 1
    assert trust[3] == 1 and stat[3, 1] == 0                                 # zero gradient
    assert 0 < trust[0] < 0.1 and 0 < trust[1] < 0.1
    c = L.clip_factor32(normsq, 5.0)
    assert c < 1                                                             # the clip is active in this case
    for t, (o, m, adapt) in enumerate(tensors):
        ew, ev = L.update32(w[o:o + m], g[o:o + m], v[o:o + m], 0.01, 0.9, c, trust[t])
        assert w2[o:o + m].tobytes() == ew.tobytes() and v2[o:o + m].tobytes() == ev.tobytes()
    assert stat[1, 0] == L.norms64(L.slot_sums32(w[8:8 + 4097])) and stat[1, 1] == L.norms64(L.slot_sums32(g[8:8 + 4097]))
    # the loss-scaled form: a non-finite norm changes nothing
    for bad in (np.inf, np.nan):
        w3, v3, t3, s3 = L.step32(w, g, v, tensors, (0.01, 0.9, 5.0), bad, 0.001, guard=True)
        assert w3.tobytes() == w.tobytes() and v3.tobytes() == v.tobytes() and t3 is None and s3 is None


def test_summary():
    assert L.summary({}) is None
    rep = {("a", "kernel"): (1.0, 2.0, 0.5), ("b", "kernel"): (1.0, 2.0, 0.125), ("c", "kernel"): (1.0, 2.0, 2.0)}
    assert L.summary(rep) == {"min": 0.125, "median": 0.5, "max": 2.0, "tensors": 3}
    rep[("d", "kernel")] = (0.0, 0.0, 1.0)
    assert L.summary(rep) == {"min": 0.125, "median": 0.75, "max": 2.0, "tensors": 4}


# ------------------------------------------------------------------ the entry points
def test_header_declares_and_bindings_hold_the_entry_points():
    import ursonet_amd.hip as hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ursonet_ext.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(urso_[a-z0-9_]+)\s*\(", txt))
    assert NAMES <= declared and len(declared) == 14
    assert NAMES <= set(hip.SIDE_SYMBOLS["ext"]) and not NAMES & set(hip.EXPORTED_SYMBOLS) and not NAMES & set(hip.LOSS_SCALE_SYMBOLS)
    assert re.search(r"#define\s+URSO_LARS_CHUNK\s+4096\b", txt)
    lib = hip.side_lib("ext")
    assert all(hasattr(lib, nm) for nm in NAMES)


def _i64(vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*vals)


def test_host_planning():
    import ursonet_amd.hip as hip
    lib = hip.side_lib("ext")
    assert lib.urso_lars_blocks(0, None) == 0
    sizes = [1, 3, 4, 5, 255, 1023, 4096, 4097, 2 * 4096 + 4, 3 * 4096, 0, 2 ** 33]
    n_h = _i64(sizes)
    nb = lib.urso_lars_blocks(len(sizes), n_h)
    assert nb == sum(L.chunks(n) for n in sizes) == 6 + 1 + 2 + 3 + 3 + 2 ** 21
    small = sizes[:-1]
    nb = lib.urso_lars_blocks(len(small), n_h)
    blockmap = np.full((nb, 2), -7, dtype=np.int32)
    first = np.full(len(small) + 1, -7, dtype=np.int32)
    assert lib.urso_lars_plan(len(small), n_h, nb, blockmap.ctypes.data, first.ctypes.data) == 0
    want = [(t, c) for t, n in enumerate(small) for c in range(L.chunks(n))]
    assert blockmap.tolist() == [list(p) for p in want]
    assert first.tolist() == list(np.cumsum([0] + [L.chunks(n) for n in small]))
    # refusals of the two host functions
    for args, msg in [((-1, n_h), "T must be >= 0"), ((2, None), "null"), ((2, _i64([5, -1])), "negative size"),
                      ((2, _i64([2 ** 62, 2 ** 62])), "2^31")]:
        assert lib.urso_lars_blocks(*args) == -1, args
        err = hip.last_error()
        assert err.startswith("urso_lars_blocks:") and msg in err, (args, err)
    B, F = blockmap.ctypes.data, first.ctypes.data
    for args, msg in [((-1, n_h, 0, B, F), "T must be >= 0"), ((len(small), None, nb, B, F), "null"), ((len(small), n_h, nb, None, F), "null"),
                      ((len(small), n_h, nb, B, None), "null"), ((len(small), n_h, nb - 1, B, F), "nblocks"),
                      ((len(small), n_h, nb + 1, B, F), "nblocks"), ((2, _i64([5, -1]), 1, B, F), "negative size")]:
        assert lib.urso_lars_plan(*args) == -1, args
        err = hip.last_error()
        assert err.startswith("urso_lars_plan:") and msg in err, (args, err)
    assert lib.urso_lars_plan(0, None, 0, None, F) == 0 and first[0] == 0    # T = 0: an empty map, first = [0]


def test_argument_validation_without_gpu():
    """Every refusal of the three launches.  Device pointers are made up and never dereferenced: each call is refused before a launch, or
    has T = 0 and launches nothing; the host tables are real."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("ext")
    W, G, V, TAB, MAP, PART, FIRST, ADAPT, HYP, NSQ, TR, STAT, LS = (0x10000 * k for k in range(1, 14))
    off, n = _i64([0, 8, 4108]), _i64([5, 4097, 3])
    nb = 1 + 2 + 1
    good_n = dict(T=3, off=off, n=n, tab=TAB, map=MAP, nb=nb, w=W, g=G, part=PART)
    bad_n = [(dict(w=None), "null"), (dict(g=None), "null"), (dict(tab=None), "null"), (dict(map=None), "null"), (dict(part=None), "null"),
             (dict(off=None), "null"), (dict(n=None), "null"), (dict(T=-1), "T must be >= 0"),
             (dict(off=_i64([0, 6, 4108])), "multiple of 4"), (dict(off=_i64([0, -4, 4108])), "multiple of 4"),
             (dict(n=_i64([5, -1, 3]), nb=2), "negative size"),
             (dict(w=W + 4), "16-byte aligned"), (dict(g=G + 8), "16-byte aligned"), (dict(tab=TAB + 4), "8-byte aligned"),
             (dict(part=PART + 4), "8-byte aligned"), (dict(map=MAP + 2), "4-byte aligned"),
             (dict(off=_i64([0, 4, 4108])), "overlap"), (dict(off=_i64([4108, 8, 0]), n=_i64([3, 4097, 12])), "overlap"),
             (dict(off=_i64([0, 8, 4104])), "overlap"), (dict(nb=nb - 1), "nblocks"), (dict(nb=nb + 1), "nblocks"), (dict(nb=0), "nblocks"),
             (dict(g=W), "same buffer")]

    def call_n(**kw):
        a = dict(good_n, **kw)
        return lib.urso_lars_norms(*[a[k] for k in good_n], None)
    for kw, msg in bad_n:
        assert call_n(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_lars_norms:") and msg in err, (kw, err)
    # tensors in any order are fine as long as they do not overlap; an empty tensor overlaps nothing (checked up to the launch: T = 0 below)
    good_s = dict(T=3, off=off, n=n, tab=TAB, map=MAP, nb=nb, w=W, g=G, v=V, trust=TR, hyper=HYP, normsq=NSQ, ls=None)
    bad_s = [(dict(w=None), "null"), (dict(g=None), "null"), (dict(v=None), "null"), (dict(trust=None), "null"), (dict(hyper=None), "null"),
             (dict(normsq=None), "null"), (dict(tab=None), "null"), (dict(map=None), "null"), (dict(off=None), "null"), (dict(n=None), "null"),
             (dict(T=-3), "T must be >= 0"), (dict(off=_i64([0, 10, 4108])), "multiple of 4"),
             (dict(w=W + 4), "16-byte aligned"), (dict(g=G + 4), "16-byte aligned"), (dict(v=V + 12), "16-byte aligned"),
             (dict(tab=TAB + 4), "8-byte aligned"), (dict(trust=TR + 1), "4-byte aligned"), (dict(ls=LS + 2), "4-byte aligned"),
             (dict(off=_i64([0, 4, 4108])), "overlap"), (dict(nb=nb + 2), "nblocks"),
             (dict(g=W), "three different"), (dict(v=W), "three different"), (dict(v=G), "three different")]

    def call_s(**kw):
        a = dict(good_s, **kw)
        return lib.urso_lars_sgd(*[a[k] for k in good_s], None)
    for kw, msg in bad_s:
        assert call_s(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_lars_sgd:") and msg in err, (kw, err)
    good_t = dict(T=3, first=FIRST, adapt=ADAPT, nb=nb, part=PART, hyper=HYP, normsq=NSQ, eta=0.001, eps=1e-8, clip=0, trust=TR, stat=STAT, ls=None)
    bad_t = [(dict(first=None), "null"), (dict(adapt=None), "null"), (dict(part=None), "null"), (dict(hyper=None), "null"),
             (dict(normsq=None), "null"), (dict(trust=None), "null"), (dict(stat=None), "null"), (dict(T=-1), "T must be >= 0"),
             (dict(nb=-1), "nblocks"), (dict(eta=0.0), "eta"), (dict(eta=-1.0), "eta"), (dict(eta=float("nan")), "eta"),
             (dict(eta=float("inf")), "eta"), (dict(eps=-1e-9), "eps"), (dict(eps=float("nan")), "eps"), (dict(clip=2), "clip_mode"),
             (dict(clip=-1), "clip_mode"), (dict(part=PART + 4), "8-byte aligned"), (dict(stat=STAT + 4), "8-byte aligned"),
             (dict(trust=TR + 2), "4-byte aligned"), (dict(first=FIRST + 1), "4-byte aligned")]

    def call_t(**kw):
        a = dict(good_t, **kw)
        return lib.urso_lars_trust(*[a[k] for k in good_t], None)
    for kw, msg in bad_t:
        assert call_t(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_lars_trust:") and msg in err, (kw, err)
    # T = 0 is valid and launches nothing (so it needs no GPU)
    assert lib.urso_lars_norms(0, None, None, None, None, 0, W, G, None, None) == 0
    assert lib.urso_lars_trust(0, None, None, 0, None, HYP, NSQ, 0.001, 0.0, 1, None, None, None, None) == 0
    assert lib.urso_lars_sgd(0, None, None, None, None, 0, W, G, V, None, HYP, NSQ, None, None) == 0
    # so do tensors that are all empty
    assert lib.urso_lars_norms(2, _i64([0, 0]), _i64([0, 0]), None, None, 0, W, G, None, None) == 0


def test_module_imports_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = "import sys; import ursonet_amd.lars; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
