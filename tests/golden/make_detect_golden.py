#!/usr/bin/env python3
"""Golden records of the reference's dataset inspection, by CALLING its own functions with recording stand-ins for matplotlib:
utils.visualize_weights, utils.visualize_axes, utils.polar_plot and a full pose_estimator.detect_dataset (pose_estimator.py:462-604).

Runs only in the build container (needs the reference tree); tests/golden/detect_dataset.npz is committed and is the only thing that
travels -- it holds data only.  The reference is imported with stub modules as make_eval_golden.py does; then `plt` (in utils and in
pose_estimator), `Circle` and `print` (in pose_estimator) are replaced by recorders, so that what the reference hands to imshow, ax.arrow,
ax.plot, Circle and print is stored as it is, not parsed from text:
  weights_n<n>/...   the slices and vmax of every imshow call of visualize_weights (GT slices first), n = 3 and 4
  axes/...           (c, v) of the three ax.arrow calls of visualize_axes for random poses; half of them passed through se3lib.quat_inv
                     first, as detect_dataset does for dataset.name == 'Speed'
  polar/...          the angles polar_plot plots (radians) for pairs of quaternions, the two pole branches of quat2euler among them
  run_<case>/...     a full detect_dataset on a stub model and dataset (`random` seeded with the stored seed): the inputs, the ids it
                     drew, the seven printed values per image and the circle centres.  Cases: the four orientation heads
                     (quaternion, Euler, angle-axis, soft classification) with a regressed location, and a 'Speed' dataset.
The reference's detect_dataset cannot finish an image with the location-classification head: its loc_est is then a 1 x 3 np.matrix, on
which utils.visualize_axes (np.transpose([C]): "shape too large to be a matrix") and loc_est[2] (:582) raise.  main() shows that it
raises and stores no such run; the blue disc of that head is checked against the closed form (tests/detectref.py) instead.

    python tests/golden/make_detect_golden.py
"""
import os
import random
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, OUT)
from make_eval_golden import BETA, Cfg, import_reference  # noqa: E402

H0, W0 = 96, 128
NR_IMAGES = 4


class Rec(object):
    """Stands in for matplotlib.pyplot, a figure and an axis at once: every call is logged as (name, args, kwargs)."""

    def __init__(self, log):
        self.log = log

    def subplots(self, *a, **kw):
        self.log.append(("subplots", a, kw))
        return (Rec(self.log), (Rec(self.log), Rec(self.log))) if a else (Rec(self.log), Rec(self.log))

    def __getattr__(self, name):
        def call(*a, **kw):
            self.log.append((name, a, kw))
            return Rec(self.log)
        return call


class Camera(object):
    def __init__(self):
        self.fx = W0 / (2 * np.tan(np.pi / 4))
        self.fy = -H0 / (2 * np.tan(73.7 * np.pi / 360))


class Data(object):
    def __init__(self, name, loc_gt, q_gt, hq=None, hmap=None):
        self.name, self.camera = name, Camera()
        self.image_ids = np.arange(len(loc_gt))
        self.image_info = [{"path": "golden://%d" % i} for i in self.image_ids]
        self.loc_gt, self.q_gt = loc_gt, q_gt
        self.ori_histogram_map, self.histogram_3D_map = hq, hmap

    def load_location(self, i):
        return self.loc_gt[i]

    def load_quaternion(self, i):
        return self.q_gt[i]

    def load_image(self, i):
        image = np.zeros((H0, W0, 3), dtype=np.uint16)
        image[0, 0, 0] = i
        return image


class Model(object):
    def __init__(self, config, outs):
        self.config, self.outs = config, outs

    def detect(self, images, verbose=0):
        return [self.outs[int(images[0][0, 0, 0])]]


def main():
    sys.path.insert(0, ROOT)
    from ursonet_amd.pose import OrientationCodec, location_map
    pe, se3lib, rutils = import_reference()
    rng = np.random.default_rng(20261018)
    f32 = lambda a: np.asarray(a, dtype=np.float32)                     # noqa: E731
    f64 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)  # noqa: E731
    store = {"beta": BETA, "frame": np.array([H0, W0])}

    def rq(n):
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        q[q[:, 3] < 0] *= -1
        return q

    def locs(n):
        return np.stack([rng.uniform(-1, 1, n), rng.uniform(-1, 1, n), rng.uniform(3, 40, n)], 1)

    # --- visualize_weights
    for n in (3, 4):
        c = OrientationCodec(n, BETA)
        gt = c.encode(rq(1))[0]
        est = rutils.stable_softmax(f32(np.log(gt.astype(np.float64) + 1e-4) + rng.normal(scale=0.7, size=gt.shape)))
        log = []
        rutils.plt = Rec(log)
        rutils.visualize_weights(gt, est, n)
        shows = [e for e in log if e[0] == "imshow"]
        assert len(shows) == 2 * n and all(e[2]["vmin"] == 0 for e in shows)
        store["weights_n%d/gt" % n], store["weights_n%d/est" % n] = f32(gt), f32(est)
        store["weights_n%d/slices" % n] = np.stack([np.asarray(e[1][0]) for e in shows])         # [2n, n, n] float32
        store["weights_n%d/vmax" % n] = np.array([e[2]["vmax"] for e in shows], dtype=np.float64)

    # --- visualize_axes
    n = 8
    q, t = rq(n), locs(n)
    inverted = np.arange(n) % 2 == 1
    K = np.matrix([[Camera().fx, 0, W0 / 2], [0, Camera().fy, H0 / 2], [0, 0, 1]])
    cs, vs = [], []
    for i in range(n):
        log = []
        rutils.visualize_axes(Rec(log), se3lib.quat_inv(q[i]) if inverted[i] else q[i], t[i], K, 100)
        arrows = [e for e in log if e[0] == "arrow"]
        assert len(arrows) == 3 and [e[2]["color"] for e in arrows] == ["r", "g", "b"]
        assert all(e[1][:2] == arrows[0][1][:2] for e in arrows)
        cs.append([float(arrows[0][1][0]), float(arrows[0][1][1])])
        vs.append([[float(e[1][2]) for e in arrows], [float(e[1][3]) for e in arrows]])
    store["axes/q"], store["axes/loc"], store["axes/inverted"], store["axes/K"] = q, t, inverted, np.asarray(K)
    store["axes/c"], store["axes/v"] = np.array(cs), np.array(vs)                                 # [n,2], [n,2,3]

    # --- polar_plot: random pairs, and one quaternion at each pole branch (x z + y w beyond +-0.499)
    q1, q2 = rq(6), rq(6)
    s = np.sqrt(0.5)
    q1[0], q1[1] = [0.0, s, 0.0, s], [0.0, -s, 0.0, s]
    q1[2] = [0.05, s, 0.02, s] / np.linalg.norm([0.05, s, 0.02, s])
    angles = []
    for a, b in zip(q1, q2):
        log = []
        rutils.plt = Rec(log)
        rutils.polar_plot(a, b)
        plots = [e for e in log if e[0] == "plot"]
        assert len(plots) == 6
        angles.append([[float(plots[2 * k][1][0][0]) for k in range(3)], [float(plots[2 * k + 1][1][0][0]) for k in range(3)]])
    store["polar/q1"], store["polar/q2"], store["polar/angles"] = q1, q2, np.array(angles)         # [6, 2 (q1, q2), 3] radians

    # --- full runs
    names = []

    def run(name, cfg, outs, tgts, data, seed):
        def load_image_gt(dataset, config, image_id):
            return (None, None) + tuple(tgts[image_id])
        sys.modules["net"].load_image_gt = load_image_gt
        pe.net = sys.modules["net"]
        log, printed, circles = [], [], []
        pe.plt = rutils.plt = Rec(log)
        pe.print = lambda *a: printed.append(a)
        pe.Circle = lambda xy, r, **kw: circles.append((xy, r, kw)) or ("circle", len(circles))
        random.seed(seed)
        with np.errstate(all="ignore"):
            if not cfg.REGRESS_LOC:
                try:
                    pe.detect_dataset(Model(cfg, outs), data, NR_IMAGES)
                except (ValueError, IndexError) as e:
                    print("%-14s the reference raises %s: %s -- not stored" % (name, type(e).__name__, e))
                    return
                raise AssertionError("the reference finished a location-classification run: store it")
            pe.detect_dataset(Model(cfg, outs), data, NR_IMAGES)
        assert len(printed) == 7 * NR_IMAGES
        c = "run_" + name
        names.append(name)
        labels = [p[0] for p in printed[:7]]
        per = [printed[7 * i:7 * i + 7] for i in range(NR_IMAGES)]
        ids = [int(p[2][1].split("//")[1]) for p in per]
        store[c + "/seed"], store[c + "/n_dataset"], store[c + "/ids"] = seed, len(data.image_ids), np.array(ids)
        store[c + "/labels"] = np.array(labels)
        store[c + "/config"] = np.array([cfg.REGRESS_LOC, cfg.REGRESS_ORI], dtype=np.int32)
        store[c + "/ori_param"], store[c + "/dataset_name"] = cfg.ORIENTATION_PARAM, data.name
        store[c + "/loc_gt"], store[c + "/q_gt"] = np.asarray(data.loc_gt), np.asarray(data.q_gt)
        store[c + "/loc_out"] = f32([o["loc"] for o in outs])
        store[c + "/ori_out"] = f32([o["ori"] for o in outs])
        flat = lambda v: np.asarray(v, dtype=np.float64).ravel()        # noqa: E731
        store[c + "/print_loc_gt"] = np.array([flat(p[0][1]) for p in per])
        store[c + "/print_loc_est"] = np.array([flat(p[1][1]) for p in per])
        store[c + "/print_q_est"] = np.array([flat(p[3][1]) for p in per])
        store[c + "/print_q_gt"] = np.array([flat(p[4][1]) for p in per])
        store[c + "/print_loc_err"] = np.array([float(p[5][1]) for p in per])
        store[c + "/print_ori_err"] = np.array([float(np.asarray(p[6][1]).ravel()[0]) for p in per])
        k = len(circles) // NR_IMAGES
        assert k in (2, 3) and len(circles) == k * NR_IMAGES
        store[c + "/circle_xy"] = np.array([[float(v) for v in xy] for xy, r, kw in circles]).reshape(NR_IMAGES, k, 2)
        store[c + "/circle_r"] = np.array([r for xy, r, kw in circles]).reshape(NR_IMAGES, k)
        store[c + "/circle_colour"] = np.array([kw["facecolor"] for xy, r, kw in circles]).reshape(NR_IMAGES, k)
        if not cfg.REGRESS_LOC:
            store[c + "/enc_loc"] = f32([t[0] for t in tgts])
        if not cfg.REGRESS_ORI:
            store[c + "/enc_ori"] = f32([t[1] for t in tgts])
            store[c + "/ori_bins"] = cfg.ORI_BINS_PER_DIM
            shows = [e for e in log if e[0] == "imshow" and "vmax" in e[2]]
            assert len(shows) == 2 * cfg.ORI_BINS_PER_DIM * NR_IMAGES
        print("%-14s ids %s" % (name, ids))

    N = 6
    for name, param, ds_name in (("quaternion", "quaternion", "Urso"), ("euler", "euler_angles", "Urso"), ("angle_axis", "angle_axis", "Urso"),
                                 ("speed", "quaternion", "Speed")):
        q_gt, loc_gt = rq(N), locs(N)
        l_o = f64(loc_gt + rng.normal(scale=0.3, size=(N, 3)))
        if param == "quaternion":
            o = rq(N)
        elif param == "euler_angles":
            o = rng.uniform(-80, 80, size=(N, 3))
        else:
            o = rng.normal(size=(N, 3))
        o = f64(o)
        outs = [{"loc": l_o[i], "ori": o[i]} for i in range(N)]
        run(name, Cfg(ORIENTATION_PARAM=param), outs, [(l_o[i], o[i]) for i in range(N)], Data(ds_name, loc_gt, q_gt), 7 + len(names))

    for name, loc_class in (("soft", False), ("soft_loc_class", True)):
        nb, m = 4, 4
        c = OrientationCodec(nb, BETA)
        q_gt, loc_gt = rq(N), locs(N)
        enc = c.encode(q_gt)
        logits = f32(np.log(enc.astype(np.float64) + 1e-4) + rng.normal(scale=0.5, size=enc.shape))
        hmap = None
        if loc_class:
            xyz = np.stack([loc_gt[:, 0] / loc_gt[:, 2], loc_gt[:, 1] / loc_gt[:, 2], loc_gt[:, 2]], 1)
            mx, mn = xyz.max(0) + 0.05, xyz.min(0) - 0.05
            hmap = location_map(m, mx, mn)
            enc_l = f32(rutils.encode_loc(xyz, m, BETA, mx, mn)[0])
            ll = f32(np.log(enc_l.astype(np.float64) + 1e-4) + rng.normal(scale=0.3, size=enc_l.shape))
            outs = [{"loc": ll[i], "ori": logits[i]} for i in range(N)]
            tgts = [(enc_l[i], enc[i]) for i in range(N)]
        else:
            l_o = f64(loc_gt + rng.normal(scale=0.3, size=(N, 3)))
            outs = [{"loc": l_o[i], "ori": logits[i]} for i in range(N)]
            tgts = [(l_o[i], enc[i]) for i in range(N)]
        run(name, Cfg(REGRESS_ORI=False, REGRESS_LOC=not loc_class, ORI_BINS_PER_DIM=nb), outs, tgts,
            Data("Urso", loc_gt, q_gt, c.H_quat, hmap), 7 + len(names))

    store["runs"] = np.array(names)
    path = os.path.join(OUT, "detect_dataset.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
