"""The weights' moving average without a GPU (Config.WEIGHT_EMA, ursonet_amd/weight_ema.py): the configuration rules, next_state (the written
specification of the one-thread kernel behind urso_ema_update) over scripted updates, update32 against a float64 evaluation, the two entry
points' surface and argument checks (they run before any launch), and the checkpoint names."""
import os
import re

import numpy as np
import pytest

from ursonet_amd import weight_ema as WE
from ursonet_amd.config import Config
from util import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ------------------------------------------------------------------ configuration
def test_defaults_off_and_inference_ignores_the_key():
    c = Config()
    assert c.WEIGHT_EMA is None and c.WEIGHT_EMA_WARMUP is True
    assert WE.initial_state(c) is None and not WE.enabled(c, "training") and not WE.enabled(c, "inference")
    on = _cfg(WEIGHT_EMA=0.999)
    assert WE.enabled(on, "training") and not WE.enabled(on, "inference")
    assert not WE.enabled(_cfg(WEIGHT_EMA="nonsense"), "inference")          # inference never looks at the value
    s = WE.initial_state(on)
    assert len(s) == WE.FIELDS == 8 and s[WE.DECAY] == float(f32(0.999)) and s[WE.WARMUP] == 1.0 and s[WE.UPDATES] == 0.0
    assert s[WE.NEXT_DECAY] == float(f32(1.0) / f32(10.0)) and s[4:] == [0.0] * 4
    s = WE.initial_state(_cfg(WEIGHT_EMA=0.999, WEIGHT_EMA_WARMUP=False))
    assert s[WE.WARMUP] == 0.0 and s[WE.NEXT_DECAY] == s[WE.DECAY] == float(f32(0.999))


@pytest.mark.parametrize("bad", [0.0, 1.0, -0.1, 1.5, True, False, float("nan"), float("inf"), "0.9", 1.0 - 1e-12, 1e-60, [0.9]])
def test_bad_decay_is_refused(bad):
    with pytest.raises(ValueError, match="WEIGHT_EMA"):
        WE.initial_state(_cfg(WEIGHT_EMA=bad))


def test_bad_warmup_and_data_parallel_are_refused(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="WEIGHT_EMA_WARMUP"):
        WE.initial_state(_cfg(WEIGHT_EMA=0.9, WEIGHT_EMA_WARMUP=1))
    with pytest.raises(ValueError, match="WEIGHT_EMA.*data parallelism"):
        WE.initial_state(_cfg(WEIGHT_EMA=0.9), world=2)
    assert WE.initial_state(_cfg(), world=2) is None                         # off: nothing to refuse
    # the data-parallel wrapper refuses an engine that keeps an average, beside its two other refusals (a stub engine: the refusals come
    # before the wrapper touches anything else of it)
    import types
    from ursonet_amd import dp
    monkeypatch.setattr(dp.dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(ValueError, match="WEIGHT_EMA.*data parallelism.*world size 2"):
        dp.DataParallelEngine(types.SimpleNamespace(ls_state=None, learn_lw=False, ema_state=object()), comm_cus=0)
    # at build, through the model: a bad key is refused before any engine exists (so this needs no GPU)
    from ursonet_amd.net import UrsoNet
    cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
    cfg.WEIGHT_EMA = 2.0
    with pytest.raises(ValueError, match="WEIGHT_EMA"):
        UrsoNet("training", cfg, str(tmp_path), build_engine=True)


def test_layout_matches_the_header_and_the_bindings():
    import ursonet_amd.hip as hip
    hdr = open(os.path.join(ROOT, "include", "ursonet_ext.h")).read()
    names = {"URSO_EMA_DECAY": WE.DECAY, "URSO_EMA_WARMUP": WE.WARMUP, "URSO_EMA_UPDATES": WE.UPDATES, "URSO_EMA_NEXT_DECAY": WE.NEXT_DECAY,
             "URSO_EMA_FIELDS": WE.FIELDS}
    for n, v in names.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % n, hdr)
        assert m and int(m.group(1)) == v, n
        assert getattr(hip, n[len("URSO_"):]) == v


# ------------------------------------------------------------------ next_state
def _run(state, n, skipped=False):
    out = []
    for _ in range(n):
        state = WE.next_state(state, skipped)
        out.append(state)
    return out


def test_next_state_over_30_updates_with_warmup():
    s0 = WE.initial_state(_cfg(WEIGHT_EMA=0.5))
    seq = _run(s0, 30)
    assert [s[WE.UPDATES] for s in seq] == [float(t) for t in range(1, 31)]
    ramp = decay = 0
    for s in seq:
        t = s[WE.UPDATES]
        q = f32(1.0 + t) / f32(10.0 + t)                                     # small integers: exact operands, one rounding
        assert float(q) == float(f32(np.float64(1.0 + t) / np.float64(10.0 + t)))      # = the float64 quotient rounded once
        assert s[WE.NEXT_DECAY] == float(min(f32(0.5), q))
        assert s[WE.DECAY] == 0.5 and s[WE.WARMUP] == 1.0 and s[4:] == [0.0] * 4
        ramp += s[WE.NEXT_DECAY] < 0.5
        decay += q > 0.5
    assert ramp == 7 and decay == 22 and seq[7][WE.NEXT_DECAY] == 0.5        # both branches; the knee is at t = 8: (1 + 8) / (10 + 8) = 1/2
    assert s0 == WE.initial_state(_cfg(WEIGHT_EMA=0.5))                      # the input is not modified
    assert WE.as_dict(seq[2]) == {"decay": 0.5, "warmup": True, "updates": 3, "next_decay": float(f32(4.0) / f32(13.0))}


def test_next_state_without_warmup_saturation_and_skip():
    seq = _run(WE.initial_state(_cfg(WEIGHT_EMA=0.5, WEIGHT_EMA_WARMUP=False)), 30)
    assert [s[WE.UPDATES] for s in seq] == [float(t) for t in range(1, 31)] and all(s[WE.NEXT_DECAY] == 0.5 for s in seq)
    for warm in (True, False):
        d = float(f32(0.9999))
        s = [d, float(warm), 2.0 ** 24 - 1, d, 0.0, 0.0, 0.0, 0.0]
        a = WE.next_state(s)
        b = WE.next_state(a)
        assert a[WE.UPDATES] == b[WE.UPDATES] == 2.0 ** 24 and a[WE.NEXT_DECAY] == b[WE.NEXT_DECAY] == d
        s[WE.UPDATES] = 2.0 ** 24                                            # set there directly
        assert WE.next_state(s) == s
    s0 = WE.initial_state(_cfg(WEIGHT_EMA=0.5))
    s3 = _run(s0, 3)[-1]
    assert WE.next_state(s3, skipped=True) == s3 and WE.next_state(s0, skipped=True) == s0
    assert _run(s3, 5, skipped=True)[-1] == s3


# ------------------------------------------------------------------ update32
def test_update32_against_float64():
    """ema + c (w - ema) with c = fl32(1 - d), the header's c.  The exact value lies between ema and w, so with M = max(|ema|, |w|) and
    u = ulp(M): |w - ema| <= 2 M, its rounding errs by at most ulp(2 M) / 2 = u; the product (c < 1) carries at most that u on and adds a
    rounding of its own of at most u; the sum is at most M in magnitude (plus those errors) and its rounding adds at most u: 3 u."""
    rng = np.random.default_rng(5)
    n = 200000
    ema = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(f32)
    w = (ema.astype(np.float64) * rng.uniform(-2, 2, size=n) + rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, size=n)).astype(f32)
    for d in (0.1, 0.5, 0.9, 0.999, 0.9999, float(f32(1.0) / f32(10.0))):
        c = f32(1.0) - f32(d)
        got = WE.update32(ema, w, d)
        assert got.dtype == f32
        want = ema.astype(np.float64) + np.float64(c) * (w.astype(np.float64) - ema.astype(np.float64))
        ulp = np.spacing(np.maximum(np.abs(ema), np.abs(w))).astype(np.float64)
        worst = float(np.max(np.abs(got.astype(np.float64) - want) / ulp))
        print("d = %-10g worst error %.3f ulp of the largest operand" % (d, worst))
        assert worst <= 3.0
    # w == ema: the difference is exactly 0 and ema keeps its bits, -0.0 and infinities aside (inf - inf is NaN: nothing is guarded)
    e = np.concatenate([ema, f32([0.0, 1e-45, 3.4e38, -1e-38])])
    assert np.array_equal(WE.update32(e, e.copy(), 0.9999).view(np.int32), e.view(np.int32))
    # special values pass through as IEEE has them
    out = WE.update32(f32([1.0, 1.0, np.inf, 2.0]), f32([np.nan, np.inf, 1.0, -np.inf]), 0.5)
    assert np.isnan(out[0]) and out[1] == np.inf and np.isnan(out[2]) and out[3] == -np.inf


# ------------------------------------------------------------------ the library's surface
def test_header_declares_and_bindings_hold_the_entry_points():
    import ursonet_amd.hip as hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ursonet_ext.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+urso_ema_update\s*\(\s*int64_t n, const float\* w_d, float\* ema_d, float\* state_d, const float\* ls_state_d, void\* stream\)", txt)
    assert re.search(r"\bint\s+urso_ema_swap\s*\(\s*int64_t n, float\* a_d, float\* b_d, void\* stream\)", txt)
    assert {"urso_ema_update", "urso_ema_swap"} <= set(hip.SIDE_SYMBOLS["ext"])
    assert not {"urso_ema_update", "urso_ema_swap"} & set(hip.EXPORTED_SYMBOLS)
    from ursonet_amd import build
    assert "weight_ema.hip" in build.SIDE_SOURCES["ext"] and os.path.exists(os.path.join(build.side_srcdir("ext"), "weight_ema.hip"))


def test_argument_validation_without_gpu():
    import ursonet_amd.hip as hip
    lib = hip.side_lib("ext")
    P, Q, S, L = 4096, 8192, 12288, 16384                                    # never dereferenced: every case fails validation or launches nothing
    bad_update = [((8, None, Q, S, None), "null"), ((8, P, None, S, None), "null"), ((8, P, Q, None, None), "null"),
                  ((-1, P, Q, S, None), "n must be >= 0"), ((-2 ** 40, P, Q, S, L), "n must be >= 0"),
                  ((8, P + 1, Q, S, None), "aligned"), ((8, P, Q + 2, S, None), "aligned"), ((8, P, Q, S + 3, None), "aligned"),
                  ((8, P, Q, S, L + 1), "aligned")]
    for args, msg in bad_update:
        assert lib.urso_ema_update(*args, None) == -1, args
        err = hip.last_error()
        assert err.startswith("urso_ema_update:") and msg in err, (args, err)
    bad_swap = [((8, None, Q), "null"), ((8, P, None), "null"), ((8, P, P), "same buffer"), ((-1, P, Q), "n must be >= 0"),
                ((8, P + 2, Q), "aligned"), ((8, P, Q + 1), "aligned")]
    for args, msg in bad_swap:
        assert lib.urso_ema_swap(*args, None) == -1, args
        err = hip.last_error()
        assert err.startswith("urso_ema_swap:") and msg in err, (args, err)
    # n = 0 is valid and launches nothing (so it needs no GPU); 4-byte alignment is enough
    assert lib.urso_ema_update(0, P, Q, S, None, None) == 0 and lib.urso_ema_update(0, P + 4, Q + 8, S, L, None) == 0
    assert lib.urso_ema_swap(0, P, Q, None) == 0 and lib.urso_ema_swap(0, P + 4, Q + 12, None) == 0


def test_module_imports_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = "import sys; import ursonet_amd.weight_ema; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


# ------------------------------------------------------------------ checkpoint names
def test_the_averaged_checkpoint_does_not_hide_the_raw_one(tmp_path):
    from ursonet_amd import net
    cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
    cfg.NAME = "x"
    m = net.UrsoNet("training", cfg, str(tmp_path), build_engine=False)
    run = tmp_path / "x20260101T0000"
    run.mkdir()
    raw = str(run / "weights_x_0002.h5")
    assert net.ema_checkpoint_path(raw) == str(run / "ema_weights_x_0002.h5")
    for name in ("weights_x_0001.h5", "ema_weights_x_0001.h5", "weights_x_0002.h5", "ema_weights_x_0002.h5", "ema_weights_x_0003.h5"):
        (run / name).write_bytes(b"")
    assert m.find_last() == (str(run), raw)
    assert m.get_last_checkpoint("x20260101T0000") == (str(run), raw)
    # the raw file's name still carries the epoch for set_log_dir, and so does the averaged one's
    m.set_log_dir(raw)
    assert m.epoch == 2 and m.checkpoint_path.format(epoch=3) == str(run / "weights_x_0003.h5")
