"""Loss scaling without a GPU: next_state (the written specification of urso_loss_scale_update) over scripted sequences of finite
and non-finite steps, and the validation of the Config.LOSS_SCALE keys (ursonet_amd/loss_scale.py)."""
import math

import pytest

from ursonet_amd import loss_scale as LS
from ursonet_amd.config import Config


def _cfg(**kw):
    c = Config()
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _run(state, script):
    out = []
    for finite in script:
        state = LS.next_state(state, finite)
        out.append(state)
    return out


def test_layout_matches_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "ursonet_loss_scale.h")).read()
    names = {"URSO_LS_SCALE": LS.SCALE, "URSO_LS_INV_SCALE": LS.INV_SCALE, "URSO_LS_GOOD_STEPS": LS.GOOD_STEPS,
             "URSO_LS_GROWTH_INTERVAL": LS.GROWTH_INTERVAL, "URSO_LS_MIN": LS.MIN, "URSO_LS_MAX": LS.MAX,
             "URSO_LS_SKIPPED_TOTAL": LS.SKIPPED_TOTAL, "URSO_LS_LAST_SKIPPED": LS.LAST_SKIPPED, "URSO_LS_FIELDS": LS.FIELDS}
    for n, v in names.items():
        m = re.search(r"\b%s\s*=\s*(\d+)" % n, hdr)
        assert m and int(m.group(1)) == v, n
    assert len(LS.FIELD_NAMES) == LS.FIELDS == 8


def test_defaults_and_off():
    c = Config()
    assert c.LOSS_SCALE is None and LS.initial_state(c) is None
    assert (c.LOSS_SCALE_INIT, c.LOSS_SCALE_GROWTH_INTERVAL, c.LOSS_SCALE_MIN, c.LOSS_SCALE_MAX) == (2.0 ** 15, 2000, 1.0, 2.0 ** 24)
    s = LS.initial_state(_cfg(LOSS_SCALE="dynamic"))
    assert s == [2.0 ** 15, 2.0 ** -15, 0.0, 2000.0, 1.0, 2.0 ** 24, 0.0, 0.0]
    s = LS.initial_state(_cfg(LOSS_SCALE=1024))
    assert s == [1024.0, 1.0 / 1024, 0.0, 0.0, 1024.0, 1024.0, 0.0, 0.0]
    assert LS.initial_state(_cfg(LOSS_SCALE=0.25))[LS.SCALE] == 0.25          # any power of two, below 1 included


def test_halving_floor_growth_cap_and_counters():
    s0 = LS.initial_state(_cfg(LOSS_SCALE="dynamic", LOSS_SCALE_INIT=8.0, LOSS_SCALE_MIN=2.0, LOSS_SCALE_MAX=16.0, LOSS_SCALE_GROWTH_INTERVAL=3))
    script = [True, True, True,          # exactly growth_interval finite steps: 8 -> 16 on the third, not before
              True, True, True,          # 16 is the cap
              False, False, False,       # 8, 4, 2
              False,                     # the floor
              True, True]                # two good steps: not yet
    seq = _run(s0, script)
    assert [s[LS.SCALE] for s in seq] == [8, 8, 16, 16, 16, 16, 8, 4, 2, 2, 2, 2]
    assert [s[LS.GOOD_STEPS] for s in seq] == [1, 2, 0, 1, 2, 0, 0, 0, 0, 0, 1, 2]
    assert [s[LS.SKIPPED_TOTAL] for s in seq] == [0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 4, 4]
    assert [s[LS.LAST_SKIPPED] for s in seq] == [0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0]
    for s in seq:
        assert s[LS.INV_SCALE] * s[LS.SCALE] == 1.0 and LS.is_power_of_two(s[LS.SCALE])
        assert (s[LS.GROWTH_INTERVAL], s[LS.MIN], s[LS.MAX]) == (3.0, 2.0, 16.0)
    # a skipped step restarts the count: finite, finite, SKIP, finite, finite, finite -> growth only after three in a row
    seq = _run(s0, [True, True, False, True, True, True])
    assert [s[LS.SCALE] for s in seq] == [8, 8, 4, 4, 4, 8]
    # the input is not modified
    assert s0 == LS.initial_state(_cfg(LOSS_SCALE="dynamic", LOSS_SCALE_INIT=8.0, LOSS_SCALE_MIN=2.0, LOSS_SCALE_MAX=16.0, LOSS_SCALE_GROWTH_INTERVAL=3))


def test_static_mode_never_moves_but_records_skips():
    s0 = LS.initial_state(_cfg(LOSS_SCALE=1024.0))
    seq = _run(s0, [True, False, False, True, True, True, True, False])
    assert all(s[LS.SCALE] == 1024.0 and s[LS.INV_SCALE] == 1.0 / 1024 for s in seq)
    assert [s[LS.SKIPPED_TOTAL] for s in seq] == [0, 1, 2, 2, 2, 2, 2, 3]
    assert [s[LS.LAST_SKIPPED] for s in seq] == [0, 1, 1, 0, 0, 0, 0, 1]
    assert LS.as_dict(seq[-1]) == {"scale": 1024.0, "skipped_total": 3, "last_step_skipped": True, "good_steps": 0}


@pytest.mark.parametrize("bad", [1000, 3.0, 0, 0.0, -2, -1024.0, float("inf"), float("nan"), True, "static", "Dynamic", [1024]])
def test_bad_static_scale_is_refused(bad):
    with pytest.raises(ValueError):
        LS.initial_state(_cfg(LOSS_SCALE=bad))


@pytest.mark.parametrize("kw", [dict(LOSS_SCALE_INIT=1000.0), dict(LOSS_SCALE_INIT=0), dict(LOSS_SCALE_INIT=-4.0),
                                dict(LOSS_SCALE_MIN=3.0), dict(LOSS_SCALE_MAX=100.0),
                                dict(LOSS_SCALE_INIT=4.0, LOSS_SCALE_MIN=8.0), dict(LOSS_SCALE_INIT=2.0 ** 20, LOSS_SCALE_MAX=2.0 ** 16),
                                dict(LOSS_SCALE_GROWTH_INTERVAL=0), dict(LOSS_SCALE_GROWTH_INTERVAL=2.5), dict(LOSS_SCALE_GROWTH_INTERVAL=-1)])
def test_bad_dynamic_keys_are_refused(kw):
    with pytest.raises(ValueError):
        LS.initial_state(_cfg(LOSS_SCALE="dynamic", **kw))


def test_scales_outside_the_fp32_normal_range_are_refused():
    """The state is fp32 and holds the reciprocal: 2**-150 would be scale 0 / inv_scale inf on the device, 2**130 scale inf, and 2**127 has a
    subnormal reciprocal.  [2**-126, 2**126] is accepted, everything beyond refused, for the static scale and for each dynamic key."""
    import struct
    for k in (-126, 126):
        s = LS.initial_state(_cfg(LOSS_SCALE=2.0 ** k))
        for v in (s[LS.SCALE], s[LS.INV_SCALE]):
            f = struct.unpack("f", struct.pack("f", v))[0]
            assert f == v and 2.0 ** -126 <= f < float("inf")              # exact and normal in fp32
        assert LS.initial_state(_cfg(LOSS_SCALE="dynamic", LOSS_SCALE_INIT=2.0 ** k, LOSS_SCALE_MIN=2.0 ** -126, LOSS_SCALE_MAX=2.0 ** 126))
    for k in (-150, -127, 127, 130):
        with pytest.raises(ValueError, match="fp32"):
            LS.initial_state(_cfg(LOSS_SCALE=2.0 ** k))
        for kw in (dict(LOSS_SCALE_INIT=2.0 ** k, LOSS_SCALE_MIN=2.0 ** -140, LOSS_SCALE_MAX=2.0 ** 140),
                   dict(LOSS_SCALE_MIN=2.0 ** k) if k < 0 else dict(LOSS_SCALE_MAX=2.0 ** k)):
            with pytest.raises(ValueError, match="fp32"):
                LS.initial_state(_cfg(LOSS_SCALE="dynamic", **kw))


def test_dynamic_is_accepted_and_world_above_one_is_refused():
    c = _cfg(LOSS_SCALE="dynamic")
    assert LS.initial_state(c, world=1)[LS.GROWTH_INTERVAL] == 2000.0
    for cfg in (c, _cfg(LOSS_SCALE=1024.0)):
        with pytest.raises(ValueError, match="data parallel"):
            LS.initial_state(cfg, world=2)
    assert LS.initial_state(Config(), world=8) is None          # off: nothing to refuse
    with pytest.raises(ValueError):
        LS.initial_state(_cfg(LOSS_SCALE=1024.0, DP_EXACT_REL_LOSS=True))


def test_power_of_two_predicate():
    for k in (-30, -1, 0, 1, 15, 24, 100):
        assert LS.is_power_of_two(math.ldexp(1.0, k))
    for v in (0, -1.0, 3, 1000, 0.3, float("inf"), float("nan"), "8", None):
        assert not LS.is_power_of_two(v)


def test_config_display_and_dump_carry_the_keys(tmp_path, capsys):
    c = _cfg(LOSS_SCALE="dynamic")
    c.display()
    out = capsys.readouterr().out
    assert "LOSS_SCALE " in out and "LOSS_SCALE_GROWTH_INTERVAL" in out
    import json
    c.write_to_file(str(tmp_path / "cfg.json"))
    d = json.load(open(str(tmp_path / "cfg.json")))
    assert d["LOSS_SCALE"] == "dynamic" and d["LOSS_SCALE_INIT"] == 32768.0


def test_extension_header_bindings_and_library_agree():
    """include/ursonet_loss_scale.h declares exactly the ten entry points hip.py binds beside the main table, the library exports each of
    them, the main header includes the extension, and the library exports nothing that neither header declares."""
    import ctypes
    import os
    import re
    import subprocess
    import ursonet_amd.hip as hip
    want = {"urso_softmax_xent_fwd_bwd_ls", "urso_rel_l2_fwd_bwd_ls", "urso_absdot_fwd_bwd_ls", "urso_mse_fwd_bwd_ls",
            "urso_param_batch_run_ls", "urso_param_grad_finalize_ls", "urso_bn_backward_ls", "urso_sgd_momentum_clip_ls",
            "urso_adam_amsgrad_clip_ls", "urso_loss_scale_update"}
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ursonet_loss_scale.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(urso_[a-z0-9_]+)\s*\(", txt)) == want == set(hip.LOSS_SCALE_SYMBOLS)
    assert not want & set(hip.EXPORTED_SYMBOLS)
    assert '#include "ursonet_loss_scale.h"' in open(os.path.join(root, "include", "ursonet_hip.h")).read()
    lib = ctypes.CDLL(hip.LIB_PATH)
    for n in want:
        assert hasattr(lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", hip.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = set(l.split()[-1] for l in out.splitlines() if " T urso_" in l)
    assert exported == want | set(hip.EXPORTED_SYMBOLS), exported ^ (want | set(hip.EXPORTED_SYMBOLS))


def test_argument_checks_need_no_device():
    import ursonet_amd.hip as hip
    # argument checks that need no device
    assert hip._lib.urso_loss_scale_update(None, None, None) != 0 and "urso_loss_scale_update" in hip.last_error()
    assert hip._lib.urso_sgd_momentum_clip_ls(4, None, None, None, None, None, None, None) != 0
