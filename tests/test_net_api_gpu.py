"""Drop-in API on the GPU: net.UrsoNet train / detect / weights round trip / batched decode, written
the way pose_estimator.py drives the reference (pose_estimator.py:747-758, 321-445, 875-913)."""
import os

import numpy as np
import pytest
import torch

from util import make_config

pytestmark = pytest.mark.gpu


def test_train_checkpoint_resume_and_detect(tmp_path):
    from ursonet_amd import net, utils
    from ursonet_amd.dataset import SyntheticPoses
    cfg = make_config("resnet18", 64, 128, batch=4, regress_ori=False, ori_bins=4, dtype="float32", lr=0.01)
    cfg.NAME = "syn"
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 6, 2
    ds_train, ds_val = SyntheticPoses(16, 64, 128, cfg, seed=1), SyntheticPoses(8, 64, 128, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=2, layers="all")
    assert len(hist.ori_loss_acc) == 12 and len(hist.loc_loss_acc) == 12 and np.isfinite(hist.ori_loss_acc).all()
    assert np.mean(hist.ori_loss_acc[-3:]) < np.mean(hist.ori_loss_acc[:3])          # it learns on 16 images
    assert model.epoch == 2
    ddir, ck = model.find_last()
    assert ck.endswith("weights_syn_0002.npz") and os.path.exists(ck)
    # resume bookkeeping (pose_estimator.py:889-913)
    m2 = net.UrsoNet(mode="inference", config=_inference_cfg(cfg), model_dir=str(tmp_path))
    m2.load_weights(ck, ck, by_name=True)
    assert m2.epoch == 2 and m2.log_dir == ddir
    w_tr, w_inf = model._engine.get_weights(), m2._engine.get_weights()
    assert all(np.array_equal(w_tr[l][w], w_inf[l][w]) for l in w_tr for w in w_tr[l])
    # detect: list of dicts with raw outputs; matches the training-mode forward on the same image
    img = ds_val.load_image(0)
    res = m2.detect([img], verbose=0)
    assert set(res[0]) == {"loc", "ori"} and res[0]["loc"].shape == (3,) and res[0]["ori"].shape == (64,)
    with pytest.raises(AssertionError):
        m2.detect([img, img])
    # probabilistic soft-argmax on the GPU == the reference-style host decode of the same logits
    from oracle import pose_math as P
    q_gpu = utils.decode_orientations(res[0]["ori"][None], ds_val.ori_histogram_map)[0]
    q_ref = P.decode_orientation(res[0]["ori"], ds_val.ori_histogram_map)
    assert abs(abs(float(np.dot(q_gpu, q_ref))) - 1) < 1e-5
    ang, le, esa = utils.pose_errors(res[0]["loc"], q_gpu, ds_val.load_location(0), ds_val.load_quaternion(0))
    assert np.isfinite(ang).all() and np.isfinite(esa).all()


def _inference_cfg(cfg):
    import copy
    c = copy.copy(cfg)
    c.IMAGES_PER_GPU = 1
    c.update()
    return c


def test_detect_matches_oracle_forward_on_uint8_image(tmp_path):
    from oracle import graph_ref as G
    from ursonet_amd import net
    cfg = make_config("resnet50", 64, 128, batch=1, regress_ori=True, dtype="float32")
    cfg.NAME = "x"
    model = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    img = np.random.default_rng(0).integers(0, 256, size=(64, 128, 3), dtype=np.uint8)
    out = model.detect([img])[0]
    P = G.to_torch(model._engine.get_weights(), requires_grad=False)
    loc, ori = G.forward(P, torch.tensor(G.mold_image(img, cfg)[None].astype(np.float32)), cfg)
    assert np.abs(out["loc"] - loc.numpy()[0]).max() < 1e-3 * np.abs(loc.numpy()).max()
    assert np.abs(out["ori"] - ori.numpy()[0]).max() < 1e-3


def test_f16_config_runs_fp16_path():
    """cfg5-style: F16=True selects the fp16 MFMA kernels (net.py:590-593 switches Keras to float16)."""
    from ursonet_amd.engine import Engine
    from oracle import graph_ref as G
    from util import synthetic_batch
    cfg = make_config("resnet50", 64, 128, batch=2, regress_ori=False, regress_loc=False, ori_bins=4, loc_bins=4, f16=True)
    eng = Engine(cfg, "training", seed=2, randomize_bn=True)
    assert eng.dt_name == "float16"
    img, loc, ori, _ = synthetic_batch(cfg, 2, seed=3)
    w0 = eng.get_weights()
    eng.load_batch(img, loc, ori); eng.step(); torch.cuda.synchronize()
    ref_l, ref_o = G.forward(G.to_torch(w0, requires_grad=False), torch.tensor(img), cfg)
    gl, go = eng.outputs()
    assert torch.isfinite(gl).all() and torch.isfinite(go).all()
    assert float((go.cpu() - ref_o).abs().max() / ref_o.abs().max()) < 5e-2


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("backbone", ["resnet18", "resnet50"])
def test_uint8_input_path_equals_molded_float_path(backbone, dtype):
    """Engine.load_batch_u8 (mean subtraction inside urso_mold_images, net.py:1337-1348) gives bit-identical network inputs and
    outputs to molding on the host, in every engine dtype (the 16-bit ones round the molded value inside the kernel); detect() and the
    other commands take that path for uint8 frames."""
    from ursonet_amd.engine import Engine
    cfg = make_config(backbone, 64, 128, batch=3, regress_ori=True, dtype=dtype)
    eng = Engine(cfg, "inference", seed=4, randomize_bn=True)
    rng = np.random.default_rng(1)
    u8 = rng.integers(0, 256, size=(3, 64, 128, 3), dtype=np.uint8)
    eng.load_batch(u8.astype(np.float32) - np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)); eng.forward(); torch.cuda.synchronize()
    a = [t.clone() for t in eng.outputs()]
    x0 = eng.acts[eng.graph.tensors[0].id]
    xa = x0.data.clone()
    eng.load_batch_u8(u8); eng.forward(); torch.cuda.synchronize()
    b = eng.outputs()
    assert torch.equal(xa, x0.data) and float(xa.float().abs().max()) > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool(torch.isfinite(a[0]).all())
    eng.set_input_u8(False)
    eng.load_batch(u8.astype(np.float32) - np.asarray(cfg.MEAN_PIXEL, dtype=np.float32)); eng.forward(); torch.cuda.synchronize()
    assert torch.equal(a[0], eng.outputs()[0])


def test_device_feeder_delivers_the_generator_batches_in_order():
    """ursonet_amd.feeder.DeviceFeeder (pinned uint8 batches, side-stream upload, double buffer) must put exactly the batches of
    the reference-format generator into the engine, in order -- frames (after the device-side mean subtraction) and targets."""
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    from ursonet_amd.engine import Engine
    from ursonet_amd.feeder import DeviceFeeder
    cfg = make_config("resnet18", 64, 128, batch=4, regress_ori=False, ori_bins=4, dtype="float32")
    ds = SyntheticPoses(10, 64, 128, cfg, seed=7)
    eng = Engine(cfg, "training", seed=1)
    feed = DeviceFeeder(eng, ds, cfg, shuffle=False, workers=3)
    gen = net.data_generator(ds, cfg, shuffle=False, batch_size=4)
    mean = torch.tensor(np.asarray(cfg.MEAN_PIXEL, dtype=np.float32), device="cuda")
    for _ in range(4):
        (imgs, meta, locs, oris), _o = next(gen)
        feed.next_into()
        torch.cuda.synchronize()
        assert float((eng.in_images_u8.float() - mean - torch.as_tensor(imgs).cuda()).abs().max()) < 1e-4      # float64 vs float32 mean subtraction
        assert torch.equal(eng.gt_loc.cpu(), torch.as_tensor(locs)) and torch.equal(eng.gt_ori.cpu(), torch.as_tensor(oris))
        eng.step()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in eng.losses().values())
    feed.close()


def test_keras_h5_weight_files_through_a_stand_in_h5py(tmp_path, monkeypatch):
    """load_weights / save_weights on Keras .h5 files (net.py:816-852): h5py is not installed in this image, so the branch is
    executed against a minimal in-memory stand-in that implements the h5py calls it makes (File, attrs, groups, datasets): the
    layer_names / weight_names attributes (bytes), the nested 'model_weights' group of full-model files and by-name matching."""
    import sys
    import types
    from ursonet_amd import net
    store = {}

    class Node(dict):
        def __init__(self):
            super(Node, self).__init__()
            self.attrs = {}

        def create_group(self, name):
            self[name] = Node(); return self[name]

        def create_dataset(self, name, data):
            self[name] = np.array(data)

    class File(Node):
        def __init__(self, path, mode="r"):
            super(File, self).__init__()
            self.path, self.mode = path, mode
            if mode == "r":
                root = store[path]
                self.update(root); self.attrs = root.attrs

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            if self.mode == "w":
                store[self.path] = self
            return False
    monkeypatch.setitem(sys.modules, "h5py", types.SimpleNamespace(File=File))
    cfg = make_config("resnet18", 64, 64, batch=1, regress_ori=True, dtype="float32")
    cfg.NAME = "h5"
    m = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    w0 = m._engine.get_weights()
    path = str(tmp_path / "weights_h5_0001.h5")
    written = net.write_weights_file(path, w0)
    assert path in written and path in store
    f = store[path]
    assert f.attrs["layer_names"][0] == b"conv0" and f["conv0"].attrs["weight_names"][0] == b"conv0/kernel:0"
    back = net.read_weights_file(path)
    assert all(np.array_equal(back[l][w], w0[l][w]) for l in w0 for w in w0[l])
    # a full-model file keeps the layers under 'model_weights' (net.py:831-832)
    nested = Node(); nested["model_weights"] = store[path]; store["nested.h5"] = nested
    back2 = net.read_weights_file("nested.h5")
    assert list(back2) == list(w0)
    m2 = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    m2._engine.set_weights({l: {w: np.zeros_like(a) for w, a in ws.items()} for l, ws in w0.items()})
    m2.load_weights(path, path, by_name=True)
    w2 = m2._engine.get_weights()
    assert all(np.array_equal(w2[l][w], w0[l][w]) for l in w0 for w in w0[l])


def test_keras_h5_weight_files_through_the_hdf5_library(tmp_path):
    """The same calls on REAL HDF5 files (no stand-in): this interpreter has no h5py, so load_weights / the checkpoint writer go through the
    HDF5 C library (ursonet_amd/h5lite.py; tests/test_h5_cpu.py pins it against files written by the real h5py).  A whole model's weights
    written to `weights_<name>_0001.h5`, read back by name into a zeroed model, checked value for value; `find_last` then finds the checkpoint
    the way the reference's resume logic does (net.py:768-800); and where an interpreter with h5py exists, the real h5py reads the file."""
    import os
    import subprocess
    from ursonet_amd import h5lite, net
    if not h5lite.available():
        pytest.skip("no HDF5 C library on this machine")
    cfg = make_config("resnet18", 64, 64, batch=1, regress_ori=True, dtype="float32")
    cfg.NAME = "h5real"
    m = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    w0 = m._engine.get_weights()
    os.makedirs(m.log_dir, exist_ok=True)
    path = os.path.join(m.log_dir, "weights_h5real_0001.h5")
    written = net.write_weights_file(path, w0)
    assert path in written and open(path, "rb").read(4) == bytes([0x89, 0x48, 0x44, 0x46])
    back = net.read_weights_file(path)
    assert list(back) == list(w0) and all(np.array_equal(back[l][w], w0[l][w]) for l in w0 for w in w0[l])
    m2 = net.UrsoNet(mode="inference", config=cfg, model_dir=str(tmp_path))
    m2._engine.set_weights({l: {w: np.zeros_like(a) for w, a in ws.items()} for l, ws in w0.items()})
    m2.load_weights(path, path, by_name=True)
    w2 = m2._engine.get_weights()
    assert all(np.array_equal(w2[l][w], w0[l][w]) for l in w0 for w in w0[l])
    py = next((p for p in (os.environ.get("URSO_H5PY_PYTHON", ""), "/opt/conda/bin/python3.9") if p and os.path.exists(p)), None)
    if py:
        gen = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_h5_golden.py")
        r = subprocess.run([py, gen, "--dump", path], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, PYTHONPATH=""), timeout=300)
        if r.returncode == 0:
            with np.load(path + ".dump.npz") as z:
                assert len(z.files) == sum(len(ws) for ws in w0.values())
                assert all(np.array_equal(z["%s/%s" % (l, w)], w0[l][w]) for l in w0 for w in w0[l])


def test_train_with_rotation_and_sim2real_augmentation_while_the_graph_is_captured(tmp_path):
    """UrsoNet.train() starts the feeders before set_trainable() / compile() reset the step graph, so the first eng.step() captures a
    hipGraph while the producer threads run the augmentation third of load_image_gt ON THE GPU (ROT_AUG warp + re-encode kernels,
    SIM2REAL stages, device-to-host copies, pinned allocations).  HIP refuses such calls from any thread during a global-mode capture:
    the producers and the capture exclude each other through hip.capture_lock.  Several capture rounds (set_trainable
    between epochs rebuilds the plan) with both augmentations on; losses stay finite and descend."""
    from ursonet_amd import net
    from ursonet_amd.dataset import SyntheticPoses
    cfg = make_config("resnet18", 64, 128, batch=4, regress_ori=False, ori_bins=4, dtype="float32", lr=0.01)
    cfg.NAME = "aug"
    cfg.ROT_AUG, cfg.SIM2REAL_AUG = True, True
    cfg.STEPS_PER_EPOCH, cfg.VALIDATION_STEPS = 5, 1
    ds_train, ds_val = SyntheticPoses(16, 64, 128, cfg, seed=1), SyntheticPoses(8, 64, 128, cfg, seed=2)
    model = net.UrsoNet(mode="training", config=cfg, model_dir=str(tmp_path))
    for layers in ("heads", "all", "4+"):                # each call rebuilds the plan and captures again with the feeders running
        hist = model.train(ds_train, ds_val, learning_rate=cfg.LEARNING_RATE, epochs=model.epoch + 1, layers=layers)
        assert len(hist.ori_loss_acc) == 5 and np.isfinite(hist.ori_loss_acc).all() and np.isfinite(hist.loc_loss_acc).all()
    assert model.epoch == 3
