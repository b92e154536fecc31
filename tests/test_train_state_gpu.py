"""The Engine's table of persistent training state (Engine.train_state) on the GPU, over a matrix of configurations
in which every optional feature of the step is on at least once (resnet18, 64 x 64, batch 2, the engine of the feature tests).

Completeness: whatever two optimizer steps change among the engine's weight-sized buffers, its `*_state` tensors and `hyper` is in the
table or is scratch that the test names.  Round trip: save, two optimizer steps, restore brings every table tensor and the micro-step
index back bit for bit, and the same two steps end in the same bits again.  Length and order: the names are the literal list of each
row, and save_train_state() is as long (one more under GRAD_ACCUM_STEPS: the host-side index)."""
import pytest
import torch

from util import make_config, synthetic_batch

pytestmark = pytest.mark.gpu

GEOM = dict(backbone="resnet18", h=64, w=64, batch=2, bottleneck=16, branch=64)
BASE = ["flat_w", "flat_v", "flat_stats"]
ADAM = ["flat_v2", "flat_vhat", "hyper"]
SCRATCH = {"flat_g", "flat_w0", "_swag_hold"}        # written by a step (or a SWAG detour) and read by no later one

# row -> (dtype, Config keys, the names of train_state() in order)
ROWS = {
    "sgd": ("float32", dict(), BASE),
    "adam": ("float32", dict(OPTIMIZER="Adam"), BASE + ADAM),
    "sgd_all": ("float32", dict(LARS=0.001, SAM=0.05, WEIGHT_EMA=0.9, SWA=1, SWA_VARIANCE=True, GRAD_ACCUM_STEPS=2),
                BASE + ["sam_state", "flat_ema", "ema_state", "flat_swa", "swa_state", "flat_swa_sq", "flat_acc"]),
    "adam_all": ("float32", dict(OPTIMIZER="Adam", LAMB=1.0, SAM=0.05, WEIGHT_EMA=0.9, SWA=1, GRAD_ACCUM_STEPS=2),
                 BASE + ADAM + ["lamb_state", "sam_state", "flat_ema", "ema_state", "flat_swa", "swa_state", "flat_acc"]),
    "fp16_loss_scale": ("float16", dict(LOSS_SCALE="dynamic", LOSS_SCALE_INIT=8.0, LOSS_SCALE_GROWTH_INTERVAL=2), BASE + ["ls_state"]),
    "learn_lw": ("float32", dict(LEARNABLE_LOSS_WEIGHTS=True), BASE),
    "bn_recal": ("float32", dict(WEIGHT_EMA=0.9, TRAIN_BN=None, BN_RECAL_BATCHES=2), BASE + ["flat_ema", "ema_state"]),
}

_engines, _batches = {}, {}


def _engine(row):
    """One engine per row, shared by the tests of the row: each leaves it a valid training engine."""
    if row not in _engines:
        from ursonet_amd.engine import Engine
        dtype, keys, _ = ROWS[row]
        cfg = make_config(dtype=dtype, **GEOM)
        for key, val in keys.items():
            setattr(cfg, key, val)
        _engines[row] = Engine(cfg, "training", seed=3, randomize_bn=True)
    return _engines[row]


def _batch(seed):
    if seed not in _batches:
        _batches[seed] = synthetic_batch(make_config(dtype="float32", **GEOM), 2, seed=seed)[:3]
    return _batches[seed]


def _two_optimizer_steps(eng):
    """Two optimizer steps: 2 k calls of step() under GRAD_ACCUM_STEPS = k, each on a batch of its own (seeds 11, 12, ...)."""
    for i in range(2 * eng.accum_k):
        eng.load_batch(*_batch(11 + i))
        eng.step()
    torch.cuda.synchronize()


def _bits(t):
    return t.detach().clone().view(torch.int32) if t.element_size() == 4 else t.detach().clone()


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("row", list(ROWS))
def test_names_order_and_length(row):
    eng, want = _engine(row), ROWS[row][2]
    table = eng.train_state()
    assert [n for n, _ in table] == want
    assert all(t is getattr(eng, n) for n, t in table)
    assert len(eng.save_train_state()) == len(want) + (1 if eng.accum_k > 1 else 0)


@pytest.mark.parametrize("row", list(ROWS))
def test_whatever_two_steps_change_is_in_the_table_or_named_scratch(row):
    eng = _engine(row)
    n = eng.flat_w.numel()
    watched = {name: t for name, t in vars(eng).items()
               if isinstance(t, torch.Tensor) and (t.numel() == n or name.endswith("_state") or name == "hyper")}
    assert {"flat_w", "flat_v", "flat_g"} <= set(watched) and set(ROWS[row][2]) - {"flat_stats"} <= set(watched)
    before = {name: _bits(t) for name, t in watched.items()}
    _two_optimizer_steps(eng)
    changed = {name for name, t in watched.items() if not _same(_bits(t), before[name])}
    print(row, "changed:", sorted(changed))
    assert {"flat_w", "flat_v", "flat_g"} <= changed                               # (the steps did move something)
    listed = {name for name, _ in eng.train_state()}
    assert changed <= listed | SCRATCH, sorted(changed - listed - SCRATCH)


@pytest.mark.parametrize("row", list(ROWS))
def test_save_two_steps_restore_is_a_round_trip(row):
    eng = _engine(row)
    eng.load_batch(*_batch(10))
    eng.step()                                                                     # (a state that no constructor leaves: mid-way under accumulation)
    torch.cuda.synchronize()
    saved = eng.save_train_state()
    start, micro = {name: _bits(t) for name, t in eng.train_state()}, eng.accum_micro
    _two_optimizer_steps(eng)
    end = {name: _bits(t) for name, t in eng.train_state()}
    assert not _same(end["flat_w"], start["flat_w"]) and eng.accum_micro == micro
    if eng.accum_k > 1:
        eng.accum_micro = (micro + 1) % eng.accum_k                                # (restore brings the index back, it does not merely leave it)
    eng.restore_train_state(saved)
    torch.cuda.synchronize()
    assert eng.accum_micro == micro
    for name, t in eng.train_state():
        assert _same(_bits(t), start[name]), name
    _two_optimizer_steps(eng)
    for name, t in eng.train_state():
        assert _same(_bits(t), end[name]), name
