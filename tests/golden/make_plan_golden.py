"""Recorder of tests/golden/plan_labels.json: the launch plan (label sequence per pass) of Engine for the configurations below, as the
engine planned them on an MI355X BEFORE the launch lists became lists of records.  tests/test_plan_golden_gpu.py rebuilds each plan
with the functions of this file and compares.  Uses only Engine(...), set_trainable, eng.labels, eng.profile_step() and a wrap of
hip.stream_ptr, so the script runs unchanged on either side of that change.

    python tests/golden/make_plan_golden.py [out.json]           # on the GPU; default: rewrites plan_labels.json

Record again (and review the diff) only when a change is MEANT to move a launch."""
import contextlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(HERE, "plan_labels.json")
PASSES = ("prep", "fwd", "loss", "bwd", "opt")
CFG2 = dict(backbone="resnet50", h=256, w=320, batch=4, regress_ori=False, ori_bins=16, dtype="bfloat16")     # the shape of the fork test
NO_FUSION_ENV = {"URSO_COMPACT_GRAD": "0", "URSO_SAMPLED_OUTPUTS": "0", "URSO_WGRAD_GROUP": "0"}
# name -> (make_config keywords, Engine mode, Engine keywords)
CONFIGS = {
    "01_resnet18": (dict(backbone="resnet18", h=128, w=128, batch=2, regress_ori=True, dtype="bfloat16"), "training", {}),
    "02_resnet50": (CFG2, "training", {}),
    "03_bench_width": (dict(CFG2, h=512, w=640, batch=2), "training", {}),
    "04_float32": (dict(backbone="resnet50", h=64, w=128, batch=2, dtype="float32"), "training", {}),
    "05_train_bn": (CFG2, "training", {}),
    "06_set_trainable": (CFG2, "training", {}),
    "07_loss_scale": (dict(backbone="resnet50", h=128, w=192, batch=2, f16=True), "training", {}),
    "08_keypoints": (dict(backbone="resnet18", h=128, w=128, batch=2, keypoints=True, dtype="bfloat16"), "training", {}),
    "09_inference": (CFG2, "inference", {}),
    "10_buckets": (CFG2, "training", dict(grad_bucket_bytes=8 << 20)),
    "11_no_fusion": (CFG2, "training", {}),
    # no standard plan has the stage-2 shortcut's data + weight gradient in a launch of its own ("dgrad+wgrad:"): the entry pair takes the
    # shortcut along unless the pair's own first layer is frozen
    "13_shortcut_alone": (dict(backbone="resnet50", h=64, w=128, batch=4, regress_ori=False, ori_bins=4, dtype="bfloat16"), "training", {}),
}
SHORTCUT_ALONE = r"(?!(res|bn)2a_branch2c$).*"
FORKED = "12_forked"          # CFG2 under URSO_WGRAD_STREAM=2, planned in a process of its own (tests/workers/fork_worker.py plan)


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update(kw)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plan_of(eng):
    """{pass: [label]} of an engine, None entries dropped, the loss launches as profile_step() names them; + the count of merged
    entry data gradients.  Steps the engine once (eagerly): the labels must be one per library call, in launch order."""
    prof = [r[0] for r in eng.profile_step()]
    plan = {k: [l for l in eng.labels[k] if l is not None] for k in PASSES}
    plan["loss"] = [l for l in prof if l == "loss"]
    assert prof == [l for k in PASSES for l in plan[k]], "profile_step() labels are not the plan's, pass by pass"
    plan["n_entry_dgrad2"] = int(getattr(eng, "n_entry_dgrad2", 0))
    return plan


def engines(name):
    """(fixture key, engine) of configuration `name`, planned and ready to step (06 re-plans twice: heads only, then stage 4 and up)."""
    from util import make_config
    from ursonet_amd import hip
    from ursonet_amd.engine import Engine
    from ursonet_amd.graph import layer_regex
    kw, mode, ekw = CONFIGS[name]
    cfg = make_config(**kw)
    if name == "05_train_bn":
        cfg.TRAIN_BN = None
    if name == "07_loss_scale":
        cfg.LOSS_SCALE = "dynamic"
    with contextlib.ExitStack() as st:
        if name == "11_no_fusion":
            st.enter_context(environ(**NO_FUSION_ENV))
            st.enter_context(hip.options(pair=0, dense=0))
        st.enter_context(environ(URSO_WGRAD_STREAM="0"))
        eng = Engine(cfg, mode, seed=11, randomize_bn=True, **ekw)
        if name == "13_shortcut_alone":
            eng.set_trainable(SHORTCUT_ALONE)
        if name != "06_set_trainable":
            yield name, eng
            return
        for layers in ("heads", "4+"):
            eng.set_trainable(layer_regex(layers))
            yield "%s_%s" % (name, layers), eng


def plans(name):
    return {key: plan_of(eng) for key, eng in engines(name)}


def stream_flags(eng):
    """One character per library call of a single step_eager(): '1' = issued on eng.wgrad_stream."""
    import torch
    from ursonet_amd import hip
    side, real, flags = eng.wgrad_stream.cuda_stream, hip.stream_ptr, []

    def spy(stream=None):
        p = real(stream)
        flags.append("1" if p == side else "0")
        return p
    hip.stream_ptr = spy
    try:
        eng.step_eager()
        torch.cuda.synchronize()
    finally:
        hip.stream_ptr = real
    return "".join(flags)


def forked_plan_here():
    """Body of `fork_worker.py plan`: this process must be a fresh one."""
    from util import make_config
    from ursonet_amd.engine import Engine
    with environ(URSO_WGRAD_STREAM="2"):
        eng = Engine(make_config(**CFG2), "training", seed=11, randomize_bn=True)
    plan = plan_of(eng)
    plan["on_side_stream"] = stream_flags(eng)
    eng._single_chain_always = True
    plan["on_side_stream_single_chain"] = stream_flags(eng)
    return plan


def forked_plan():
    """FORKED's plan from a fresh child process, started as tests/test_model_gpu.py::_fork_worker starts its workers."""
    env = dict(os.environ)
    env.pop("URSO_WGRAD_STREAM", None)
    p = subprocess.run([sys.executable, os.path.join(TESTS, "workers", "fork_worker.py"), "plan"], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=600)
    out = p.stdout.decode(errors="replace")
    assert p.returncode == 0, "fork worker failed (rc %d):\n%s" % (p.returncode, out[-3000:])
    return json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])


def main(path=FIXTURE):
    fixture = {}
    for name in CONFIGS:
        fixture.update(plans(name))
        print("recorded", name, flush=True)
    fixture[FORKED] = forked_plan()
    with open(path, "w") as f:
        json.dump(fixture, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s: %d plans, %d bytes" % (path, len(fixture), os.path.getsize(path)))


if __name__ == "__main__":
    main(*sys.argv[1:2])
