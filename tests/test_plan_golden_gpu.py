"""The launch plan of Engine for fourteen configurations against tests/golden/plan_labels.json, recorded on an MI355X before the launch
lists became lists of records (tests/golden/make_plan_golden.py holds the configurations and the recorder): the same launches, under the
same labels, in the same order, pass by pass -- and, for the forked plan, the same launches on the side stream."""
import json
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_plan_golden as G      # noqa: E402

with open(G.FIXTURE) as _f:
    GOLDEN = json.load(_f)

NAME = r"[^+:@]+"
# every form of launch the planner's rewrites produce must occur in the fixture: a fixture without one pins nothing about that rewrite
FORMS = {
    "fwd:a+b": r"fwd:res%s\+res%s" % (NAME, NAME),
    "fwd:a+s+b": r"fwd:%s\+%s\+%s" % (NAME, NAME, NAME),
    "@sampled": r"fwd:%s@sampled" % NAME,
    "+sampled": r"fwd:%s\+sampled" % NAME,
    "fwd:...+maxpool": r"fwd:%s\+maxpool" % NAME,
    "dgrad:a+b+wgrad:b": r"dgrad:%s\+(%s)\+wgrad:\1" % (NAME, NAME),
    "dgrad+wgrad:": r"dgrad\+wgrad:%s" % NAME,
    "grouped wgrad:a+b...": r"wgrad:%s(\+(?!maxpool_bwd)%s)+" % (NAME, NAME),
    "wgrad:...+maxpool_bwd": r"wgrad:%s\+maxpool_bwd" % NAME,
    "dgrad_heads:": r"dgrad_heads:.+",
    "wgrad_heads:": r"wgrad_heads:.+",
    "reduce:bucket": r"reduce:bucket\d+",
    "loss_scale": r"loss_scale",
}


def _deferral_point(plan):
    """(index in the backward labels of the first stage-3 / stage-2 data gradient, side-stream flags of the backward launches)."""
    bwd = plan["bwd"]
    off = len(plan["prep"]) + len(plan["fwd"]) + len(plan["loss"])
    assert len(plan["on_side_stream"]) == off + len(bwd) + len(plan["opt"]), "one flag per launch"
    return next(i for i, l in enumerate(bwd) if re.match(r"dgrad:res[23]", l)), plan["on_side_stream"][off:off + len(bwd)]


def test_the_fixture_holds_every_form_of_launch():
    assert os.path.getsize(G.FIXTURE) < 100 * 1000
    assert sorted(GOLDEN) == sorted([n for n in G.CONFIGS if n != "06_set_trainable"] + ["06_set_trainable_heads", "06_set_trainable_4+", G.FORKED])
    labels = [l for plan in GOLDEN.values() for k in G.PASSES for l in plan[k]]
    assert all(isinstance(l, str) for l in labels)
    for form, rx in FORMS.items():
        assert any(re.fullmatch(rx, l) for l in labels), "no launch of the form %s in the fixture" % form
    assert any(plan["n_entry_dgrad2"] >= 1 for plan in GOLDEN.values())         # a plan that merged a stage's two entry data gradients
    assert len(set(l for l in GOLDEN["10_buckets"]["bwd"] if l.startswith("reduce:"))) > 1                  # several gradient buckets
    forked = GOLDEN[G.FORKED]
    at, side = _deferral_point(forked)
    assert "1" in side[at:], "no launch on the side stream behind the deferral point"
    moved = len(side[:at]) - len(side[:at].rstrip("1"))                          # the side-stream launches that stand right in front of the point
    assert moved >= 3 and all(l.startswith("wgrad") for l in forked["bwd"][at - moved:at])
    assert forked["bwd"] != GOLDEN["02_resnet50"]["bwd"] and sorted(forked["bwd"]) == sorted(GOLDEN["02_resnet50"]["bwd"])
    assert set(forked["on_side_stream"][:len(forked["on_side_stream"]) - len(side) - len(forked["opt"])]) == {"0"}      # nothing but backward launches
    assert set(forked["on_side_stream_single_chain"]) == {"0"} and len(forked["on_side_stream_single_chain"]) == len(forked["on_side_stream"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.CONFIGS))
def test_plan_is_the_recorded_one(name):
    for key, plan in G.plans(name).items():
        for k in G.PASSES + ("n_entry_dgrad2",):
            assert plan[k] == GOLDEN[key][k], (key, k)


@pytest.mark.gpu
def test_forked_plan_and_its_side_stream_launches_are_the_recorded_ones():
    """In a process of its own (tests/workers/fork_worker.py plan): the labels after the reordering, which launches of one eager step run
    on the side stream, and none of them once the engine has fallen back to the single chain."""
    plan = G.forked_plan()
    assert plan == GOLDEN[G.FORKED], [k for k in GOLDEN[G.FORKED] if plan.get(k) != GOLDEN[G.FORKED][k]]
