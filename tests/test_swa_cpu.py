"""Stochastic weight averaging and SWAG-diagonal without a GPU (Config.SWA, ursonet_amd/swa.py): the configuration rules and every refusal,
next_state (the written specification of the one-thread kernel behind urso_swa_update) over the edges of start and period, collect32
against a float64 running mean, the first-model copy and the never-moving-weight invariants, Philox-4x32-10 against the Random123 known
answers, the moments of the reference normals, sample32's fixed points, and the two entry points' surface and argument checks (they run
before any launch)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from libsurface import header_symbols
from ursonet_amd import swa as S
from ursonet_amd.config import Config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_train.h")
SWA_NAMES = {"urso_swa_update", "urso_swag_sample"}
f32 = np.float32


def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------ configuration
def test_defaults_off_and_inference_ignores_the_key():
    c = Config()
    assert c.SWA is None and c.SWA_START == 0 and c.SWA_VARIANCE is False and c.SWA_RECAL_BATCHES == 0
    assert S.validate(c) is None and S.initial_state(c) is None and not S.enabled(c, "training") and not S.enabled(c, "inference")
    on = _cfg(SWA=4, SWA_START=3, SWA_VARIANCE=True)
    assert S.enabled(on, "training") and not S.enabled(on, "inference")
    assert S.validate(on) == (4, 3, True, 0)
    s = S.initial_state(on)
    assert s == [4, 3, 0, 0, 0, 1, 0, 0] and len(s) == S.FIELDS == 8
    assert S.initial_state(_cfg(SWA=1)) == [1, 0, 0, 0, 0, 0, 0, 0]
    assert S.initial_state(_cfg(SWA=np.int64(7), SWA_START=np.int32(2))) == [7, 2, 0, 0, 0, 0, 0, 0]
    assert S.as_dict(s) == {"period": 4, "start": 3, "ticks": 0, "models": 0, "collected": False, "variance": True}
    assert S.validate(_cfg(SWA=2, SWA_RECAL_BATCHES=3, TRAIN_BN=None)) == (2, 0, False, 3)


@pytest.mark.parametrize("bad", [0, -1, True, False, "4", b"4", 2.5, float("nan"), float("inf"), -float("inf"), [4], 2 ** 31, 1e30])
def test_bad_period_is_refused(bad):
    with pytest.raises(ValueError, match=r"^SWA must be None or an int > 0"):
        S.initial_state(_cfg(SWA=bad))


@pytest.mark.parametrize("bad", [-1, True, "0", 0.5, float("nan"), float("inf"), None, 2 ** 31])
def test_bad_start_and_recal_batches_are_refused(bad):
    with pytest.raises(ValueError, match=r"^SWA_START must be an int >= 0"):
        S.initial_state(_cfg(SWA=4, SWA_START=bad))
    with pytest.raises(ValueError, match=r"^SWA_START must be an int >= 0"):
        S.validate(_cfg(SWA_START=bad))                                      # also with the feature off: a key is well formed or refused
    with pytest.raises(ValueError, match=r"^SWA_RECAL_BATCHES must be an int >= 0"):
        S.validate(_cfg(SWA=4, SWA_RECAL_BATCHES=bad, TRAIN_BN=None))


@pytest.mark.parametrize("bad", [1, 0, "True", None, 1.0])
def test_bad_variance_is_refused(bad):
    with pytest.raises(ValueError, match=r"^SWA_VARIANCE must be True or False"):
        S.initial_state(_cfg(SWA=4, SWA_VARIANCE=bad))


def test_recal_batches_need_the_average_and_batch_statistics():
    with pytest.raises(ValueError, match=r"SWA_RECAL_BATCHES = 2 needs SWA"):
        S.validate(_cfg(SWA_RECAL_BATCHES=2, TRAIN_BN=None))
    with pytest.raises(ValueError, match=r"SWA_RECAL_BATCHES = 2 needs TRAIN_BN = None"):
        S.validate(_cfg(SWA=4, SWA_RECAL_BATCHES=2, TRAIN_BN=False))
    # BN_RECAL_BATCHES stays tied to WEIGHT_EMA: SWA does not satisfy it
    from ursonet_amd import bn_recal
    with pytest.raises(ValueError, match="needs WEIGHT_EMA"):
        bn_recal.validate(_cfg(SWA=4, BN_RECAL_BATCHES=2, TRAIN_BN=None))


def test_data_parallel_is_refused(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match=r"SWA is not supported under data parallelism \(world size 2\)"):
        S.initial_state(_cfg(SWA=4), world=2)
    assert S.initial_state(_cfg(), world=2) is None                          # off: nothing to refuse
    import types
    from ursonet_amd import dp
    monkeypatch.setattr(dp.dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="SWA.*data parallelism.*world size 2"):
        dp.DataParallelEngine(types.SimpleNamespace(ls_state=None, learn_lw=False, ema_state=None, swa_state=object()), comm_cus=0)
    # at build, through the model: a bad key is refused before any engine exists (so this needs no GPU)
    from ursonet_amd.net import UrsoNet
    from util import make_config
    cfg = make_config(dtype="float32", backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
    cfg.SWA = 2.5
    with pytest.raises(ValueError, match=r"^SWA must be"):
        UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    cfg.SWA = 2
    with pytest.raises(ValueError, match="SWA.*data parallelism"):
        UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))


@pytest.mark.parametrize("bad", [-0.5, float("nan"), float("inf"), True, "0.5", None, 1e80])
def test_bad_var_scale_is_refused(bad):
    with pytest.raises(ValueError, match="var_scale must be a finite float >= 0"):
        S.scale32(bad)


def test_scale_is_the_rounded_root():
    assert S.scale32() == float(f32(np.sqrt(0.5))) and S.scale32(0) == 0.0 and S.scale32(4.0) == 2.0


# ------------------------------------------------------------------ the state
def _run(state, steps, skipped=()):
    out = []
    for k in range(steps):
        state = S.next_state(state, skipped=k in skipped)
        out.append(list(state))
    return out


def test_next_state_start_zero_period_one_collects_every_step():
    rows = _run(S.initial_state(_cfg(SWA=1)), 5)
    assert [r[S.TICKS] for r in rows] == [1, 2, 3, 4, 5] and [r[S.MODELS] for r in rows] == [1, 2, 3, 4, 5]
    assert all(r[S.COLLECTED] == 1 for r in rows)


def test_next_state_first_collection_is_the_step_at_start_plus_period():
    rows = _run(S.initial_state(_cfg(SWA=4, SWA_START=3, SWA_VARIANCE=True)), 12)
    assert [r[S.TICKS] for r in rows] == list(range(1, 13))
    assert [r[S.COLLECTED] for r in rows] == [0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 0]         # steps 7 = 3 + 4 and 11
    assert [r[S.MODELS] for r in rows] == [0] * 6 + [1] * 4 + [2] * 2
    assert all(r[S.PERIOD] == 4 and r[S.START] == 3 and r[S.VARIANCE] == 1 and r[6:] == [0, 0] for r in rows)
    rows = _run(S.initial_state(_cfg(SWA=3)), 7)                             # start = 0: steps 3 and 6
    assert [r[S.COLLECTED] for r in rows] == [0, 0, 1, 0, 0, 1, 0]
    rows = _run(S.initial_state(_cfg(SWA=1, SWA_START=2)), 4)                # period 1 behind a start: every step from 3 on
    assert [r[S.COLLECTED] for r in rows] == [0, 0, 1, 1]


def test_skipped_steps_move_nothing():
    s0 = S.initial_state(_cfg(SWA=2))
    rows = _run(s0, 6, skipped={0, 3})
    assert rows[0] == s0                                                     # a skipped first step: the state of before, COLLECTED included
    assert [r[S.TICKS] for r in rows] == [0, 1, 2, 2, 3, 4]
    assert [r[S.COLLECTED] for r in rows] == [0, 0, 1, 1, 0, 1]              # step 4 was skipped: COLLECTED keeps what step 3 left
    assert [r[S.MODELS] for r in rows] == [0, 0, 1, 1, 1, 2]


def test_model_cap_and_tick_saturation():
    s = [1, 0, 100, S.MAX_MODELS - 1, 0, 0, 0, 0]
    s = S.next_state(s)
    assert s[S.MODELS] == S.MAX_MODELS == 2 ** 24 and s[S.COLLECTED] == 1
    s = S.next_state(s)
    assert s[S.MODELS] == 2 ** 24 and s[S.COLLECTED] == 0 and s[S.TICKS] == 102      # the cap: ticks go on, no model is collected
    s = S.next_state([5, 0, S.MAX_TICKS - 1, 7, 0, 0, 0, 0])
    assert s[S.TICKS] == S.MAX_TICKS == 2 ** 31 - 1
    assert S.next_state(s)[S.TICKS] == S.MAX_TICKS                           # saturated


# ------------------------------------------------------------------ the collection rule
def test_first_model_is_a_bit_copy():
    rng = np.random.default_rng(0)
    w = rng.normal(size=10 ** 5).astype(f32)
    old = rng.normal(size=10 ** 5).astype(f32)
    mean, sq = S.collect32(old, old, w, 1)
    assert np.array_equal(_bits(mean), _bits(w)) and np.array_equal(_bits(sq), _bits(w * w))
    # the reason the copy is needed: mean + (w - mean) is not w in float32
    assert int((_bits((old + (w - old).astype(f32)).astype(f32)) != _bits(w)).sum()) > 10 ** 4
    mean, sq = S.collect32(old, None, w, 1)
    assert sq is None and np.array_equal(_bits(mean), _bits(w))


def test_collect32_follows_a_float64_running_mean():
    """64 collections along a trajectory (weights over four decades that wander by a percent around their starting point, as the weights
    at the low points of a cyclic rate do): per element within n * 2^-24 relative of the float64 running mean -- a collection adds at
    most three roundings, and with |w - mean| << |mean| only the last, of the sum, is of relative size 2^-24 (half an ulp)."""
    rng = np.random.default_rng(1)
    n_el = 4096
    base = (rng.choice([-1.0, 1.0], size=n_el) * 10.0 ** rng.uniform(-2, 2, size=n_el)).astype(f32)
    mean = sq = None
    m64 = np.zeros(n_el)
    q64 = np.zeros(n_el)
    for n in range(1, 65):
        w = (base * (1.0 + 0.01 * rng.normal(size=n_el))).astype(f32)
        mean, sq = S.collect32(mean, sq if n > 1 else np.zeros(n_el, f32), w, n)
        m64 += (w.astype(np.float64) - m64) / n
        q64 += (w.astype(np.float64) ** 2 - q64) / n
        assert np.all(np.abs(mean - m64) <= n * 2.0 ** -24 * np.abs(m64)), n
        assert np.all(np.abs(sq - q64) <= n * 2.0 ** -24 * q64), n
    assert mean.dtype == np.float32 and sq.dtype == np.float32 and np.all(q64 > m64 ** 2)


def test_a_weight_that_never_moves_keeps_its_bits_and_samples_at_itself():
    rng = np.random.default_rng(2)
    w = (rng.normal(size=10 ** 4) * 10.0 ** rng.uniform(-6, 6, size=10 ** 4)).astype(f32)
    mean, sq = S.collect32(None, np.zeros_like(w), w, 1)
    for n in list(range(2, 70)) + [1000, 2 ** 24]:
        mean, sq = S.collect32(mean, sq, w, n)
        assert np.array_equal(_bits(mean), _bits(w)) and np.array_equal(_bits(sq), _bits(w * w)), n
    z = S.normals(w.size, seed=5, sample=1)
    assert np.array_equal(_bits(S.sample32(mean, sq, z, S.scale32(0.5))), _bits(w))          # sd is exactly 0


# ------------------------------------------------------------------ sampling
def test_philox_known_answers():
    kat = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
           ([0xffffffff] * 4, [0xffffffff] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in kat:
        got = S.philox4x32_10(np.array(ctr), np.array(key))
        assert got.dtype == np.uint32 and " ".join("%08x" % v for v in got) == want
    # vectorised: rows are independent
    got = S.philox4x32_10(np.array([k[0] for k in kat]), np.array([k[1] for k in kat]))
    assert [" ".join("%08x" % v for v in row) for row in got] == [k[2] for k in kat]
    assert S.PHILOX_M0 == 0xD2511F53 and S.PHILOX_M1 == 0xCD9E8D57 and S.PHILOX_W0 == 0x9E3779B9 and S.PHILOX_W1 == 0xBB67AE85


def test_reference_normals_have_the_moments_of_a_standard_normal():
    N = 2 ** 20
    z = S.normals64(N, seed=1234, sample=0)
    assert z.dtype == np.float64 and z.size == N and np.isfinite(z).all()
    assert abs(z.mean()) <= 5.0 / np.sqrt(N) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / N)
    assert np.abs(z).max() <= 6.8                                            # sqrt(-2 ln(2^-33)) = 6.76
    z32 = S.normals(N, seed=1234, sample=0)
    assert z32.dtype == np.float32 and np.array_equal(z32, z.astype(f32))


def test_normals_depend_on_the_absolute_index_seed_and_sample_alone():
    full = S.normals64(1003, seed=2 ** 32 + 9, sample=7)
    for first, n in ((0, 1), (4, 13), (500, 503), (996, 7), (3, 5)):
        assert np.array_equal(S.normals64(n, 2 ** 32 + 9, 7, first=first), full[first:first + n])
    assert not np.array_equal(S.normals64(16, 9, 7), full[:16])              # the high word of the seed is part of the key
    assert not np.array_equal(S.normals64(16, 2 ** 32 + 9, 6), full[:16])
    # the counter layout: element 4 i + j is word j of counter (i, 0, sample, 0) under key (seed lo, seed hi)
    x = S.philox4x32_10(np.array([3, 0, 7, 0]), np.array([9, 1]))
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    want = np.sqrt(-2.0 * np.log(u[0])) * np.array([np.cos(S.TWO_PI * u[1]), np.sin(S.TWO_PI * u[1])])
    assert np.array_equal(full[12:14], want)


def test_sample32_fixed_points_and_rule():
    rng = np.random.default_rng(3)
    mean = rng.normal(size=1000).astype(f32)
    z = S.normals(1000, 0, 0)
    sq = ((mean * mean).astype(f32) + rng.uniform(0.01, 1.0, size=1000).astype(f32)).astype(f32)
    assert np.array_equal(_bits(S.sample32(mean, sq, z, 0.0)), _bits(mean))                      # s = 0
    assert np.array_equal(_bits(S.sample32(mean, (mean * mean).astype(f32), z, 0.7)), _bits(mean))      # sq = fl(mean^2)
    assert np.array_equal(_bits(S.sample32(mean, (sq * f32(0.0)).astype(f32), z, 0.7)), _bits(mean))    # a negative difference counts as 0
    s = S.scale32(0.5)
    sd = np.sqrt((sq - (mean * mean).astype(f32)).astype(f32)).astype(f32)
    want = (mean + ((f32(s) * sd).astype(f32) * z).astype(f32)).astype(f32)
    got = S.sample32(mean, sq, z, s)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want)) and not np.array_equal(got, mean)


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == set(hip.SIDE_SYMBOLS["train"]) and SWA_NAMES <= names and "swa.hip" in build.SIDE_SOURCES["train"]
    assert re.search(r"#define\s+URSO_SWA_STATE\s+8\b", txt) and hip.SWA_STATE == S.FIELDS == 8
    for k, field in enumerate(S.FIELD_NAMES):
        assert re.search(r"#define\s+URSO_SWA_%s\s+%d\b" % (field.upper(), k), txt), field
    assert re.search(r"#define\s+URSO_SWA_MAX_MODELS\s+%d\b" % S.MAX_MODELS, txt)
    assert re.search(r"#define\s+URSO_SWA_REFUSED\s+\(%d\)" % S.REFUSED, txt)
    assert len(hip.SIDE_SIGS["train"]["urso_swa_update"][1]) == 7 and len(hip.SIDE_SIGS["train"]["urso_swag_sample"][1]) == 10


def test_argument_validation_without_gpu():
    """Every refusal of the two entry points.  Device pointers are made up and never dereferenced: each call is refused before a launch,
    or has n = 0 and launches nothing."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("train")
    W, M, Q, ST, LS, O, Z = (0x1000000 * k for k in range(1, 8))

    def call(fn, good, kw):
        a = dict(good, **kw)
        return getattr(lib, fn)(*[a[k] for k in good], None)
    good_u = dict(n=1000, w=W, mean=M, sq=Q, state=ST, ls=LS)
    distinct = "distinct buffers"
    bad_u = [(dict(w=None), "null"), (dict(mean=None), "null"), (dict(state=None), "null"),
             (dict(n=-1), "n must be >= 0"), (dict(n=-2 ** 40), "n must be >= 0"),
             (dict(w=W + 2), "4-byte aligned"), (dict(mean=M + 1), "4-byte aligned"), (dict(sq=Q + 3), "4-byte aligned"),
             (dict(state=ST + 2), "4-byte aligned"), (dict(ls=LS + 1), "4-byte aligned"),
             (dict(mean=W), distinct), (dict(sq=W), distinct), (dict(sq=M), distinct), (dict(mean=W + 3996), distinct),
             (dict(sq=M - 3996), distinct), (dict(sq=None, mean=W), distinct)]
    for kw, msg in bad_u:
        assert call("urso_swa_update", good_u, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_swa_update:") and msg in err, (kw, err)
    good_s = dict(n=1000, first=0, mean=M, sq=Q, out=O, z=Z, s=0.5, seed=7, sample=0)
    own = "buffers of their own"
    bad_s = [(dict(mean=None), "null"), (dict(sq=None), "null"), (dict(out=None), "null"),
             (dict(n=-1), "n must be >= 0"), (dict(mean=M + 2), "4-byte aligned"), (dict(sq=Q + 1), "4-byte aligned"),
             (dict(out=O + 3), "4-byte aligned"), (dict(z=Z + 2), "4-byte aligned"),
             (dict(first=-4), "first must be a multiple of 4"), (dict(first=6), "first must be a multiple of 4"),
             (dict(s=-0.5), "s must be finite and >= 0"), (dict(s=float("nan")), "s must be finite and >= 0"),
             (dict(s=float("inf")), "s must be finite and >= 0"), (dict(sample=-1), "sample must be >= 0"),
             (dict(out=M), own), (dict(out=Q), own), (dict(z=M), own), (dict(z=Q), own), (dict(z=O), own),
             (dict(out=M + 3996), own), (dict(z=O - 3996), own), (dict(out=Q - 4), own)]
    for kw, msg in bad_s:
        assert call("urso_swag_sample", good_s, kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_swag_sample:") and msg in err, (kw, err)
    # n = 0 is valid and launches nothing (so it needs no GPU), at any alignment, with and without the optional buffers
    assert lib.urso_swa_update(0, W, M + 4, Q + 8, ST, None, None) == 0 and lib.urso_swa_update(0, W, M, None, ST, LS, None) == 0
    assert lib.urso_swag_sample(0, 0, M, Q + 4, O + 8, None, 0.5, 2 ** 40, 3, None) == 0
    assert lib.urso_swag_sample(0, 8, M, Q, O, Z, 0.0, 0, 0, None) == 0
    # the refusals come in front of n == 0
    assert lib.urso_swa_update(0, W, W, None, ST, None, None) == -1 and lib.urso_swag_sample(0, 0, M, Q, M, None, 0.5, 0, 0, None) == -1


def test_checkpoint_names_stay_out_of_find_last():
    from ursonet_amd.net import swa_checkpoint_path
    p = os.path.join("logs", "run", "weights_urso_0007.h5")
    assert swa_checkpoint_path(p) == os.path.join("logs", "run", "swa_weights_urso_0007.h5")
    assert swa_checkpoint_path(p, sqmean=True) == os.path.join("logs", "run", "swa_sqmean_urso_0007.h5")
    assert not os.path.basename(swa_checkpoint_path(p)).startswith("weights")


def test_module_imports_neither_torch_nor_the_engine():
    code = ("import sys; import ursonet_amd.swa; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules "
            "and 'ursonet_amd.engine' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
