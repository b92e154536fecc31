"""Gradient accumulation without a GPU (Config.GRAD_ACCUM_STEPS, ursonet_amd/grad_accum.py): the configuration rules, the launch roles, the
folding of the per-micro-batch loss history, c = fl32(1 / k), a derived error bound of the float32 recurrence against the float64 mean, the
three entry points' surface and their argument checks (they run before any launch)."""
import os
import re

import numpy as np
import pytest

from ursonet_amd import grad_accum as GA
from ursonet_amd.config import Config
from util import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U = 2.0 ** -24                                   # unit roundoff of float32


def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


# ------------------------------------------------------------------ configuration
def test_default_is_off_and_inference_ignores_the_key():
    c = Config()
    assert c.GRAD_ACCUM_STEPS == 1 and GA.validate(c) == 1 and not GA.enabled(c, "training")
    assert GA.validate(object()) == 1                                        # a config from before the key: off
    on = _cfg(GRAD_ACCUM_STEPS=4)
    assert GA.validate(on) == 4 and GA.enabled(on, "training") and not GA.enabled(on, "inference")
    assert not GA.enabled(_cfg(GRAD_ACCUM_STEPS="nonsense"), "inference")    # inference never looks at the value
    assert GA.validate(_cfg(GRAD_ACCUM_STEPS=np.int64(3))) == 3
    assert GA.validate(_cfg(GRAD_ACCUM_STEPS=1), world=8) == 1               # off: nothing to refuse under a launcher


@pytest.mark.parametrize("bad", [True, False, 2.0, "2", 0, -1, None, 1.5, [2], np.float32(2)])
def test_bad_values_are_refused(bad):
    with pytest.raises(ValueError, match="GRAD_ACCUM_STEPS"):
        GA.validate(_cfg(GRAD_ACCUM_STEPS=bad))


def test_data_parallel_runs_and_the_model_refuse(monkeypatch, tmp_path):
    with pytest.raises(ValueError, match="GRAD_ACCUM_STEPS.*data parallelism.*world size 2"):
        GA.validate(_cfg(GRAD_ACCUM_STEPS=2), world=2)
    # the data-parallel wrapper refuses k > 1 at every world size, one rank included: it replays graph cuts of its own (a stub engine: the
    # refusals come before the wrapper touches anything else of it)
    import types
    from ursonet_amd import dp
    for world in (2, 1):
        monkeypatch.setattr(dp.dist, "get_world_size", lambda group=None, world=world: world)
        stub = types.SimpleNamespace(ls_state=None, learn_lw=False, ema_state=None, mode="training", config=_cfg(GRAD_ACCUM_STEPS=2))
        with pytest.raises(ValueError, match="GRAD_ACCUM_STEPS"):
            dp.DataParallelEngine(stub, comm_cus=0)
    # at build, through the model: a bad key is refused before any engine exists (so this needs no GPU); so is k > 1 under a launcher
    from ursonet_amd.net import UrsoNet
    for bad in (True, 2.0, "2", 0):
        cfg = make_config(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
        cfg.GRAD_ACCUM_STEPS = bad
        with pytest.raises(ValueError, match="GRAD_ACCUM_STEPS"):
            UrsoNet("training", cfg, str(tmp_path), build_engine=True)


# ------------------------------------------------------------------ roles, history, c
def test_roles():
    assert GA.roles(1) == [] and GA.ROLES == ("first", "add", "close")
    assert GA.roles(2) == ["first", "close"]
    assert GA.roles(3) == ["first", "add", "close"]
    assert GA.roles(5) == ["first", "add", "add", "add", "close"]


def test_fold_history():
    rows = np.arange(24, dtype=f32).reshape(6, 4) ** 2
    assert GA.fold_history(rows, 1) is rows
    two = GA.fold_history(rows, 2)
    assert two.dtype == f32 and two.shape == (3, 4)
    assert np.array_equal(two, ((rows[0::2].astype(np.float64) + rows[1::2]) / 2).astype(f32))
    three = GA.fold_history(rows, 3)
    assert three.shape == (2, 4) and np.array_equal(three[1], rows[3:6].astype(np.float64).mean(0).astype(f32))
    assert GA.fold_history(np.zeros((0, 4), f32), 3).shape == (0, 4)
    with pytest.raises(ValueError):
        GA.fold_history(rows, 4)
    nan = rows.copy()
    nan[2, 1] = np.nan                                                       # a non-finite micro-batch loss shows in its optimizer step alone
    assert np.isnan(GA.fold_history(nan, 2)[1, 1]) and np.isfinite(GA.fold_history(nan, 2)[[0, 2]]).all()


def test_inv32():
    for k in (2, 4, 8, 1024):
        c = GA.inv32(k)
        assert isinstance(c, f32) and float(c) == 1.0 / k                    # powers of two: exact
    for k in (3, 5, 6, 7, 100):
        c = GA.inv32(k)
        assert isinstance(c, f32) and c == f32(1.0 / k) and float(c) != 1.0 / k
        assert abs(float(c) * k - 1.0) <= U                                  # one rounding of 1 / k


# ------------------------------------------------------------------ the recurrence against the float64 mean
def _decades(shape, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=shape) * 10.0 ** rng.uniform(-6, 6, size=shape)).astype(f32)
    x[np.abs(x) < 1e-30] = 1.0
    return x


def _bound(gs, k):
    """|fl32 recurrence - float64 mean| <= gamma_(k+1) * (sum_j |g_j|) / k, gamma_m = m u / (1 - m u), u = 2^-24.
    Derivation: s_1 = g_1 is exact; s_j = fl(s_(j-1) + g_j) for j = 2 .. k are k - 1 roundings; r = fl(s_k * c) is one more, and
    c = fl(1 / k) = (1 / k)(1 + d) carries one of its own: k + 1 roundings in all.  Every g_j reaches r through at most all of them, each a
    factor (1 + d_i) with |d_i| <= u, so r = (1 / k) sum_j g_j (1 + e_j) with |e_j| <= (1 + u)^(k+1) - 1 <= gamma_(k+1).  No underflow: a
    float32 add is exact where its result is subnormal, and the products here are far above 2^-126 (one quantum, 2^-149, is added anyway)."""
    m = k + 1
    gamma = m * U / (1.0 - m * U)
    return gamma * np.sum(np.abs(np.asarray(gs, dtype=np.float64)), axis=0) / k + 2.0 ** -149


def _recurrence(gs, c):
    acc = GA.first32(gs[0])
    for g in gs[1:]:
        acc = GA.add32(acc, g)
    return (acc * f32(c)).astype(f32)


@pytest.mark.parametrize("k", [2, 3, 5, 8])
def test_the_recurrence_is_within_k_plus_1_roundings_of_the_float64_mean(k):
    n = 100000
    gs = [_decades(n, 10 * k + j) for j in range(k)]
    got = GA.accumulate32(gs)
    assert got.dtype == f32
    acc = GA.first32(gs[0])
    assert acc is not gs[0] and np.array_equal(acc.view(np.int32), gs[0].view(np.int32))
    mean = np.sum(np.asarray(gs, dtype=np.float64), axis=0) / k
    bound = _bound(gs, k)
    err = np.abs(got.astype(np.float64) - mean)
    print("k = %d: worst error / bound %.3f" % (k, float(np.max(err / bound))))
    assert (err <= bound).all()
    # the bound has teeth: a recurrence that drops a term, and one that counts a term twice, both fall outside it
    assert np.array_equal(_recurrence(gs, GA.inv32(k)).view(np.int32), got.view(np.int32))
    dropped = _recurrence(gs[:1] + gs[2:], GA.inv32(k))
    twice = _recurrence(gs[:2] + [gs[1]] + gs[2:], GA.inv32(k))
    for name, wrong in (("dropped", dropped), ("twice", twice)):
        outside = np.abs(wrong.astype(np.float64) - mean) > bound
        print("k = %d, %s: %.1f %% of the elements outside the bound" % (k, name, 100.0 * outside.mean()))
        assert outside.mean() > 0.5, name


def test_special_values_pass_through():
    inf, nan = np.inf, np.nan
    acc = GA.add32(f32([1.0, inf, inf, 3e38]), f32([nan, 1.0, -inf, 3e38]))
    assert np.isnan(acc[0]) and acc[1] == inf and np.isnan(acc[2]) and acc[3] == inf
    out = GA.close32(f32([1.0, inf, 3e38, 1.0]), f32([2.0, 1.0, 3e38, nan]), GA.inv32(2))
    assert out[0] == 1.5 and out[1] == inf and out[2] == inf and np.isnan(out[3])       # the sum overflows before the multiply: nothing is guarded


# ------------------------------------------------------------------ the library's surface
NAMES = {"urso_grad_accum", "urso_grad_accum_parts", "urso_grad_accum_close"}


def test_header_declares_and_bindings_hold_the_entry_points():
    import ursonet_amd.hip as hip
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ursonet_ext.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+urso_grad_accum\s*\(\s*int64_t n, const float\* g_d, float\* acc_d, int first, void\* stream\)", txt)
    assert re.search(r"\bint\s+urso_grad_accum_parts\s*\(\s*int64_t n\)", txt)
    assert re.search(r"\bint\s+urso_grad_accum_close\s*\(\s*int64_t n, float\* g_d, const float\* acc_d, float c, float\* sqpart_d, int nparts, "
                     r"void\* stream\)", txt)
    assert NAMES <= set(hip.SIDE_SYMBOLS["ext"]) and not NAMES & set(hip.EXPORTED_SYMBOLS)
    from ursonet_amd import build
    assert "grad_accum.hip" in build.SIDE_SOURCES["ext"] and os.path.exists(os.path.join(build.side_srcdir("ext"), "grad_accum.hip"))


def test_parts_is_the_documented_grid():
    import ursonet_amd.hip as hip
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4097, 2 ** 20 + 3, 2 ** 22 - 1, 2 ** 22, 2 ** 22 + 1, 2 ** 22 + 2 ** 12 + 1, 33554432, 2 ** 33):
        assert hip.grad_accum_parts(n) == min(4096, -(-(-(-n // 4)) // 256)), n
    assert hip.grad_accum_parts(0) == 0 and hip.grad_accum_parts(-5) == 0


def test_argument_validation_without_gpu():
    import ursonet_amd.hip as hip
    lib = hip.side_lib("ext")
    P, Q, S = 4096, 8192, 12288                                              # never dereferenced: every case fails validation or launches nothing
    bad_accum = [((8, None, Q, 0), "null"), ((8, P, None, 1), "null"), ((-1, P, Q, 0), "n must be >= 0"), ((-2 ** 40, P, Q, 1), "n must be >= 0"),
                 ((8, P + 1, Q, 0), "aligned"), ((8, P, Q + 2, 1), "aligned"), ((8, P, P, 0), "same buffer"), ((8, P, P, 1), "same buffer")]
    for args, msg in bad_accum:
        assert lib.urso_grad_accum(*args, None) == -1, args
        err = hip.last_error()
        assert err.startswith("urso_grad_accum:") and msg in err, (args, err)
    parts = hip.grad_accum_parts(5000)
    assert parts == 5
    bad_close = [((8, None, Q, 0.5, S, 1), "null"), ((8, P, None, 0.5, S, 1), "null"), ((8, P, Q, 0.5, None, 1), "null"),
                 ((-1, P, Q, 0.5, S, 0), "n must be >= 0"), ((8, P + 3, Q, 0.5, S, 1), "aligned"), ((8, P, Q + 1, 0.5, S, 1), "aligned"),
                 ((8, P, Q, 0.5, S + 2, 1), "aligned"), ((8, P, P, 0.5, S, 1), "same buffer"),
                 ((5000, P, Q, 0.5, S, parts - 1), "nparts"), ((5000, P, Q, 0.5, S, parts + 1), "nparts"), ((8, P, Q, 0.5, S, 0), "nparts"),
                 ((0, P, Q, 0.5, S, 1), "nparts")]
    for args, msg in bad_close:
        assert lib.urso_grad_accum_close(*args, None) == -1, args
        err = hip.last_error()
        assert err.startswith("urso_grad_accum_close:") and msg in err, (args, err)
    # n = 0 is valid and launches nothing (so it needs no GPU); 4-byte alignment is enough
    assert lib.urso_grad_accum(0, P, Q, 0, None) == 0 and lib.urso_grad_accum(0, P + 4, Q + 8, 1, None) == 0
    assert lib.urso_grad_accum_close(0, P, Q, 0.5, S, 0, None) == 0 and lib.urso_grad_accum_close(0, P + 4, Q + 12, 0.5, S + 4, 0, None) == 0


def test_module_imports_neither_torch_nor_the_library():
    import subprocess
    import sys
    code = "import sys; import ursonet_amd.grad_accum; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
