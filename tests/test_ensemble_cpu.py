"""Ensemble inference without a GPU (predict / evaluate / test_and_submit with members=..., ursonet_amd/ensemble.py): the closed forms of
add64 / settle64 (the NumPy float64 statement of urso_ens_add / urso_ens_settle), the Members list and every refusal of the public
interface before torch, the engine or the library is touched, the surface of liburso_train.so against header and bindings, and the two
entry points' argument checks (they run before any launch)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from libsurface import header_symbols
from ursonet_amd import ensemble as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ursonet_train.h")
ENS_NAMES = {"urso_ens_add", "urso_ens_settle"}
EPS = 2.0 ** -52
LN2 = float(np.log(2.0))


def _members(zs):
    acc = stat = None
    for z in zs:
        acc, stat = E.add64(z, acc, stat)
    return acc, stat


# ------------------------------------------------------------------ closed forms
def test_one_member_is_the_softmax():
    rng = np.random.default_rng(0)
    z = (rng.normal(size=(5, 37)) * 4).astype(np.float32)
    acc, stat = E.add64(z)
    z64 = z.astype(np.float64)
    ref = np.exp(z64 - z64.max(axis=1, keepdims=True))
    ref /= ref.sum(axis=1, keepdims=True)
    assert np.array_equal(acc, ref) and np.all(stat[:, 1] == 1) and np.all(stat[:, 2:] == 0)
    H = -(ref * np.log(ref)).sum(axis=1)
    assert np.all(np.abs(stat[:, 0] - H) <= (37 + 16) * EPS * H)
    logp, t = E.settle64(acc, stat, 1)
    assert logp.dtype == np.float32 and t.shape == (5, E.COLS)
    e = np.exp(logp.astype(np.float64))
    # softmax(logp) is pbar up to fp32 rounding: logp moves by at most |logp| 2^-24, which is a relative step of p; the sum by no more
    tol = 2.001 * np.abs(logp).max(axis=1, keepdims=True) * 2.0 ** -24
    assert np.all(np.abs(e / e.sum(axis=1, keepdims=True) - ref) <= tol * ref)
    assert np.array_equal(t[:, E.PEAK], ref.max(axis=1)) and np.array_equal(t[:, E.ARGMAX], ref.argmax(axis=1))
    assert np.all(t[:, E.N_MEMBERS] == 1) and np.all(t[:, 6:] == 0)
    assert np.all(np.abs(t[:, E.H_MEAN] - H) <= (37 + 16) * EPS * H)
    assert np.all(t[:, E.MI] >= 0) and np.all(t[:, E.MI] <= 2 * (37 + 16) * EPS * 2 * H)


def test_disjoint_one_hot_members_give_ln2():
    K = 9
    a = np.full((1, K), -np.inf, dtype=np.float32)
    b = a.copy()
    a[0, 2] = 0
    b[0, 6] = 0
    acc, stat = _members([a, b])
    assert np.array_equal(acc[0], np.eye(K)[2] + np.eye(K)[6]) and np.array_equal(stat[0], [0, 2, 0, 0])
    logp, t = E.settle64(acc, stat, 2)
    assert t[0, E.H_MEAN] == LN2 and t[0, E.H_MEMBERS] == 0 and t[0, E.MI] == LN2
    assert t[0, E.PEAK] == 0.5 and t[0, E.ARGMAX] == 2 and t[0, E.N_MEMBERS] == 2
    assert np.array_equal(logp[0, [2, 6]], np.float32([-LN2, -LN2]))
    rest = np.delete(logp[0], [2, 6])
    assert np.all(rest == -E.FLT_MAX) and np.all(np.isfinite(rest))         # a zero bin: -FLT_MAX, never -inf


@pytest.mark.parametrize("M", [1, 2, 5, 64])
def test_identical_members_have_no_mutual_information(M):
    rng = np.random.default_rng(M)
    K = 64
    z = (rng.normal(size=(4, K)) * 3).astype(np.float32)
    acc, stat = _members([z] * M)
    _logp, t = E.settle64(acc, stat, M)
    bound = (K + 16) * EPS * M * (t[:, E.H_MEAN] + t[:, E.H_MEMBERS])
    print("MI", t[:, E.MI], "bound", bound)
    assert np.all(t[:, E.MI] >= 0) and np.all(t[:, E.MI] <= bound)
    assert np.all(t[:, E.N_MEMBERS] == M)


@pytest.mark.parametrize("K", [1, 2, 63, 4096])
def test_uniform_logits_give_ln_k(K):
    z = np.full((2, K), 3.25, dtype=np.float32)
    acc, stat = _members([z, z, z])
    _logp, t = E.settle64(acc, stat, 3)
    lnk = np.log(float(K))
    tol = (K + 16) * EPS * 3 * max(lnk, 1.0)
    assert np.all(np.abs(stat[:, 0] / 3 - lnk) <= tol) and np.all(np.abs(t[:, E.H_MEAN] - lnk) <= tol)
    assert np.all(np.abs(t[:, E.PEAK] * K - 1) <= 4 * EPS) and np.all(t[:, E.ARGMAX] == 0)


def test_nan_and_inf_logits_make_nan_rows_and_touch_no_other():
    rng = np.random.default_rng(3)
    z = rng.normal(size=(4, 11)).astype(np.float32)
    z[1, 4] = np.nan
    z[2, 7] = np.inf
    z[3, 0] = -np.inf
    acc, stat = _members([z, z])
    logp, t = E.settle64(acc, stat, 2)
    for r in (1, 2):
        assert np.all(np.isnan(acc[r])) and np.isnan(stat[r, 0]) and stat[r, 1] == 2
        assert np.all(np.isnan(logp[r])) and np.all(np.isnan(t[r, :E.ARGMAX])) and t[r, E.ARGMAX] == 0
    for r in (0, 3):
        assert np.all(np.isfinite(acc[r])) and np.all(np.isfinite(t[r])) and np.all(np.isfinite(logp[r]))
    assert acc[3, 0] == 0 and logp[3, 0] == -E.FLT_MAX and abs(acc[3].sum() - 2) <= 16 * EPS
    ok = E.add64(z[[0, 3]])
    assert np.array_equal(ok[0], E.add64(z)[0][[0, 3]])                     # rows are independent


def test_mutual_information_is_clamped_at_zero_and_keeps_nan():
    acc = np.array([[0.5, 0.5], [0.5, 0.5], [np.nan, 0.5]])
    stat = np.array([[LN2 * 1.0000001, 1, 0, 0], [0.25, 1, 0, 0], [0.1, 1, 0, 0]])
    _logp, t = E.settle64(acc, stat, 1)
    assert t[0, E.MI] == 0.0 and not np.signbit(t[0, E.MI]) and t[1, E.MI] == LN2 - 0.25 and np.isnan(t[2, E.MI])
    with pytest.raises(ValueError, match="1 <= M <= 64"):
        E.settle64(acc, stat, 0)
    with pytest.raises(ValueError, match="1 <= M <= 64"):
        E.settle64(acc, stat, 65)


def test_gpu_cases_keep_the_logp_cap_under_the_bound():
    """The premise of tests/test_ensemble_gpu.py's cap on logp: for its seeds, the reference moved by the whole bound either way changes
    fl32(log(pbar)) in at most CAP of all cases' elements -- so a device result inside the bound stays under the cap too -- and the
    cases hold what they promise: a zero bin, a NaN row, finite rows beside them."""
    import ensref as R
    flips = total = 0
    for K, M, scale in R.all_cases():
        z = R.member_logits(K, M, scale)
        acc, _stat, logp, table = R.reference(z)
        f, t = R.logp_flips(acc, M, K)
        flips, total = flips + f, total + t
        if K > 1 and scale == 1.0:
            assert logp[0, K - 1] == -E.FLT_MAX and np.all(np.isfinite(table[0]))
        if K > 1 and scale == 30.0:
            assert np.all(np.isnan(logp[1])) and np.all(np.isfinite(logp[0])) and np.isnan(table[1, E.MI])
    print("flips under the bound", flips, "of", total)
    assert len(R.all_cases()) == 38 and flips <= R.CAP * total


# ------------------------------------------------------------------ the member list and the interface's refusals
def test_members_validation(tmp_path):
    good = str(tmp_path / "w_0001.npz")
    np.savez(good, **{"conv1/kernel": np.zeros(3)})
    layer = {"conv1": {"kernel": np.zeros(3)}}
    ms = E.Members([good, layer, tmp_path / "w_0001.npz"])
    assert len(ms) == 3
    assert list(ms.load(0, ["conv1"])) == ["conv1"] and np.array_equal(ms.load(1, ["conv1"])["conv1"]["kernel"], np.zeros(3))
    with pytest.raises(ValueError, match="member 0 lacks 1 layer"):
        ms.load(0, ["conv1", "fc"])
    assert len(E.Members([layer] * 64)) == 64
    for bad, msg in (([], r"1 \.\. 64 weight sets \(got 0\)"), ([layer] * 65, r"1 \.\. 64 weight sets \(got 65\)"), (good, "must be a list"),
                     (layer, "must be a list"), (None, "must be a list"), ([str(tmp_path / "absent.npz")], "member 0: no such weights file"),
                     ([good, 3], "member 1 must be a weights file path"), ([good, str(tmp_path / "w.txt")], "member 1 must be a .h5 or .npz"),
                     ([{}], "member 0 must map layer names"), ([{"conv1": np.zeros(3)}], "member 0 must map layer names")):
        with pytest.raises(ValueError, match=msg):
            E.Members(bad)
    with pytest.raises(ValueError, match=r"evaluate\(members=\.\.\.\) cannot be combined with views"):
        E.Members([good], views=[[0, 0, 10]], who="evaluate")


def test_size_check_names_the_figure():
    # 1000 images, 64^3 orientation bins: 1000 * 262144 * 8 bytes = 1.9531 GiB of accumulator alone, 1.9536 GiB with the small tables
    need = E.accumulator_bytes(1000, 4, 64 ** 3, 0, False)
    assert need == 1000 * (64 ** 3 * 8 + 96) + 4 * 1000 * 12 * 8 == 2097632000
    assert E.check_size(1000, 4, 64 ** 3, 0, False, 16) == need
    with pytest.raises(ValueError, match=r"need 1\.954 GiB on the device, more than max_gb = 1\b"):
        E.check_size(1000, 4, 64 ** 3, 0, False, 1)
    assert E.accumulator_bytes(10, 2, 8, 27, True) == 10 * (8 * 8 + 96 + 32) + 10 * (27 * 8 + 96 + 108) + 2 * 10 * 96 + 10 * 56
    for bad in (0, -1, float("nan"), None, "x"):
        with pytest.raises(ValueError, match="max_gb must be a number > 0"):
            E.check_size(10, 2, 8, 0, False, bad)


def test_interface_refuses_before_torch_the_engine_or_the_library():
    code = """
import sys
import pytest
from ursonet_amd import ensemble, evaluate, predict, submission
class Boom(object):
    def __getattr__(self, name):
        raise AssertionError("touched %s" % name)
for fn, who in ((predict.predict, "predict"), (evaluate.evaluate, "evaluate")):
    for kw, msg in ((dict(members=[]), "1 .. 64 weight sets"), (dict(members=[{"a": {}}] * 65), "1 .. 64 weight sets"),
                    (dict(members=["/nonexistent/w.npz"]), "no such weights file"), (dict(members=[7]), "must be a weights file path"),
                    (dict(members=[{"a": {}}], views=[[0, 0, 5]]), "cannot be combined with views")):
        with pytest.raises(ValueError) as err:
            fn(Boom(), Boom(), **kw)
        assert msg in str(err.value) and str(err.value).startswith(who), err.value
with pytest.raises(ValueError, match="1 .. 64 weight sets"):
    submission.test_and_submit(Boom(), Boom(), Boom(), members=[])
assert "torch" not in sys.modules and "ursonet_amd.hip" not in sys.modules and "ursonet_amd.engine" not in sys.modules
"""
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)


def test_results_without_members_carry_none():
    from ursonet_amd.evaluate import EvalResult
    from ursonet_amd.predict import PredictResult
    names = ("n_members", "member_loc_spread", "member_ori_spread", "member_lambda", "ori_entropy", "ori_member_entropy", "ori_mi",
             "loc_entropy", "loc_member_entropy", "loc_mi")
    code = "import sys; import ursonet_amd.ensemble; assert 'torch' not in sys.modules and 'ursonet_amd.hip' not in sys.modules"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    p = PredictResult([0, 1], np.zeros((2, 12)), False, False)
    e = EvalResult([0, 1], np.zeros((2, 16)), False, False, False)
    for r in (p, e):
        assert all(getattr(r, k) is None for k in names)
    with pytest.raises(TypeError):
        PredictResult([0], np.zeros((1, 12)), False, False, None, False, None)     # ensemble is keyword-only


# ------------------------------------------------------------------ the library's surface
def test_header_bindings_and_library_agree():
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names, txt = header_symbols(HEADER)
    assert names == set(hip.SIDE_SYMBOLS["train"]) and ENS_NAMES <= names and "ensemble.hip" in build.SIDE_SOURCES["train"]
    for macro, v in (("MAX_MEMBERS", E.MAX_MEMBERS), ("STAT", E.STAT), ("COLS", E.COLS), ("H_MEAN", E.H_MEAN), ("H_MEMBERS", E.H_MEMBERS),
                     ("MI", E.MI), ("PEAK", E.PEAK), ("ARGMAX", E.ARGMAX), ("N_MEMBERS", E.N_MEMBERS)):
        assert re.search(r"#define\s+URSO_ENS_%s\s+%d\b" % (macro, v), txt), macro
        assert getattr(hip, "ENS_" + macro) == v
    # the argument structs are the header's: field order and sizes
    assert [f[0] for f in hip.EnsAddArgs._fields_] == ["B", "n", "row0", "K", "ld", "first", "pad", "logits", "acc", "stat"]
    assert [f[0] for f in hip.EnsSettleArgs._fields_] == ["n", "row0", "K", "M", "acc", "stat", "logp", "table"]
    assert C.sizeof(hip.EnsAddArgs) == 56 and C.sizeof(hip.EnsSettleArgs) == 56 and hip.EnsSettleArgs.row0.offset == 8


def test_argument_validation_without_gpu():
    """Every refusal of the two entry points.  Device pointers are made up and never dereferenced: each call is refused before a launch,
    or has n = 0 and launches nothing."""
    import ursonet_amd.hip as hip
    lib = hip.side_lib("train")
    Z, A, S, L, T = (0x1000000 * k for k in range(1, 6))

    def add(**kw):
        a = hip.EnsAddArgs()
        for k, v in dict(dict(B=4, n=3, row0=0, K=8, ld=8, first=1, pad=0, logits=Z, acc=A, stat=S), **kw).items():
            setattr(a, k, v)
        return lib.urso_ens_add(C.byref(a), None)

    def settle(**kw):
        a = hip.EnsSettleArgs()
        for k, v in dict(dict(n=3, row0=0, K=8, M=2, acc=A, stat=S, logp=L, table=T), **kw).items():
            setattr(a, k, v)
        return lib.urso_ens_settle(C.byref(a), None)
    bad_add = [(dict(logits=None), "null pointer"), (dict(acc=None), "null pointer"), (dict(stat=None), "null pointer"),
               (dict(B=0), "B > 0"), (dict(B=-1), "B > 0"), (dict(n=-1), "0 <= n <= B"), (dict(n=5), "0 <= n <= B"),
               (dict(row0=-1), "row0 must be >= 0"), (dict(K=0), "K must be >= 1"), (dict(K=-3, ld=-3), "K must be >= 1"),
               (dict(ld=7), "ld 7 < K 8"), (dict(logits=Z + 2), "logits must be 4-byte aligned"),
               (dict(acc=A + 4), "acc and stat must be 8-byte aligned"), (dict(stat=S + 4), "acc and stat must be 8-byte aligned")]
    for kw, msg in bad_add:
        assert add(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_ens_add:") and msg in err, (kw, err)
    bad_settle = [(dict(acc=None), "null pointer"), (dict(stat=None), "null pointer"), (dict(logp=None), "null pointer"),
                  (dict(table=None), "null pointer"), (dict(n=-1), "n must be >= 0"), (dict(row0=-2), "row0 must be >= 0"),
                  (dict(K=0), "K must be >= 1"), (dict(M=0), "1 <= M <= 64"), (dict(M=65), "1 <= M <= 64"), (dict(M=-1), "1 <= M <= 64"),
                  (dict(logp=L + 1), "logp must be 4-byte aligned"), (dict(acc=A + 4), "8-byte aligned"), (dict(stat=S + 2), "8-byte aligned"),
                  (dict(table=T + 4), "8-byte aligned")]
    for kw, msg in bad_settle:
        assert settle(**kw) == -1, kw
        err = hip.last_error()
        assert err.startswith("urso_ens_settle:") and msg in err, (kw, err)
    assert lib.urso_ens_add(None, None) == -1 and "null argument struct" in hip.last_error()
    assert lib.urso_ens_settle(None, None) == -1 and "null argument struct" in hip.last_error()
    # n = 0 is valid and launches nothing (so it needs no GPU), at any 4- / 8-byte alignment
    assert add(n=0) == 0 and add(n=0, logits=Z + 4, acc=A + 8, first=0, ld=11) == 0 and settle(n=0) == 0 and settle(n=0, logp=L + 4, M=64) == 0
    # the refusals come in front of n == 0
    assert add(n=0, K=0) == -1 and settle(n=0, M=0) == -1
