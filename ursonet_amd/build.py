"""Builds liburso_hip.so, the extension library liburso_ext.so, the optimizer library liburso_opt.so, the training library liburso_train.so, the inference library liburso_infer.so, the feature library liburso_feat.so and the explanation library liburso_explain.so (gfx950) in-tree with hipcc.  `python -m ursonet_amd.build`."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
# Kernel experiments: URSO_LIB_VARIANT=<name> builds / loads lib/liburso_hip_<name>.so compiled with URSO_VARIANT_FLAGS
# (e.g. "-DURSO_PW_NT=1"), so that two compile-time variants can be compared inside ONE gpurun call on the same box.
VARIANT = os.environ.get("URSO_LIB_VARIANT", "")
LIB = os.path.join(LIBDIR, "liburso_hip%s.so" % (("_" + VARIANT) if VARIANT else ""))
SOURCES = ["runtime.hip", "conv_igemm.hip", "conv_pw.hip", "conv_pwx.hip", "conv_dense.hip", "conv_bneck.hip", "conv_halo.hip", "conv_halo2.hip", "conv_winograd.hip", "conv_pair.hip", "conv_pairw.hip", "conv_pairx.hip", "conv_pairs.hip", "conv_c3.hip", "conv_c3g.hip", "conv_hwgrad.hip", "conv_stem.hip", "conv_stemw.hip", "conv_wgrad.hip", "prep.hip", "pool_loss_optim.hip", "augment.hip", "resize.hip", "frame_cache.hip", "video.hip", "pmf_sheet.hip", "bn_train.hip", "comm.hip", "quat_gmm.hip", "pose_eval.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off"]
# The extension library (include/ursonet_ext.h): entry points added after liburso_hip.so's surface was frozen.  Same flags, no variant;
# it calls into the main library (error text, launch profiler), which the loader resolves when it is loaded behind it (ursonet_amd/hip.py).
CSRC_EXT = os.path.join(HERE, "csrc_ext")
EXT_LIB = os.path.join(LIBDIR, "liburso_ext.so")
EXT_SOURCES = ["pose_fuse.hip", "loss_weights.hip", "weight_ema.hip", "grad_accum.hip", "lars.hip"]
# The optimizer library (include/ursonet_opt.h): entry points added after liburso_ext.so's surface was frozen too.  Built and loaded as that one.
CSRC_OPT = os.path.join(HERE, "csrc_opt")
OPT_LIB = os.path.join(LIBDIR, "liburso_opt.so")
OPT_SOURCES = ["lamb.hip"]
# The training library (include/ursonet_train.h): training features added after liburso_opt.so's surface was frozen as well; its own surface
# stays open, so the next one goes here.  Built and loaded as the other two.
CSRC_TRAIN = os.path.join(HERE, "csrc_train")
TRAIN_LIB = os.path.join(LIBDIR, "liburso_train.so")
TRAIN_SOURCES = ["sam.hip", "bn_recal.hip", "swa.hip", "ensemble.hip", "calibrate.hip"]
# The inference library (include/ursonet_infer.h): inference features added after liburso_train.so's surface was pinned; its own surface
# stays open.  Built and loaded as the other three.
CSRC_INFER = os.path.join(HERE, "csrc_infer")
INFER_LIB = os.path.join(LIBDIR, "liburso_infer.so")
INFER_SOURCES = ["conformal.hip"]
# The feature library (include/ursonet_feat.h): feature-space statistics of the bottleneck features (ursonet_amd/domain.py); liburso_infer.so's
# surface was pinned to conformal's two names.  Built and loaded as the other four.
CSRC_FEAT = os.path.join(HERE, "csrc_feat")
FEAT_LIB = os.path.join(LIBDIR, "liburso_feat.so")
FEAT_SOURCES = ["feat.hip"]
# The explanation library (include/ursonet_explain.h): occlusion-sensitivity maps (ursonet_amd/explain.py); liburso_feat.so's surface was pinned
# to its three names.  Built and loaded as the other five.
CSRC_EXPLAIN = os.path.join(HERE, "csrc_explain")
EXPLAIN_LIB = os.path.join(LIBDIR, "liburso_explain.so")
EXPLAIN_SOURCES = ["explain.hip"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def source_hash():
    """SHA-256 over everything the library is a function of: every file of csrc/ (name + bytes), the public headers, the compile flags
    (incl. URSO_VARIANT_FLAGS) and the compiler's version string."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)) + [os.path.join(HERE, "..", "include", f) for f in ("ursonet_hip.h", "ursonet_loss_scale.h")]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(FLAGS + os.environ.get("URSO_VARIANT_FLAGS", "").split() + SOURCES).encode())
    _hash_compiler(h)
    return h.hexdigest()


def _hash_compiler(h):
    try:
        h.update(subprocess.run([_hipcc(), "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60).stdout)
    except Exception:
        pass


def _side_source_hash(srcdir, sources):
    """source_hash() of a library behind the main one: every file of its source directory, the headers of csrc/ it may include, the public
    headers, the compile flags and the compiler's version string."""
    import hashlib
    h = hashlib.sha256()
    inc = os.path.join(HERE, "..", "include")
    files = (sorted(os.path.join(srcdir, f) for f in os.listdir(srcdir)) + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) +
             sorted(os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(FLAGS + sources).encode())
    _hash_compiler(h)
    return h.hexdigest()


def ext_source_hash():
    """source_hash() of the extension library."""
    return _side_source_hash(CSRC_EXT, EXT_SOURCES)


def opt_source_hash():
    """source_hash() of the optimizer library."""
    return _side_source_hash(CSRC_OPT, OPT_SOURCES)


def train_source_hash():
    """source_hash() of the training library."""
    return _side_source_hash(CSRC_TRAIN, TRAIN_SOURCES)


def infer_source_hash():
    """source_hash() of the inference library."""
    return _side_source_hash(CSRC_INFER, INFER_SOURCES)


def feat_source_hash():
    """source_hash() of the feature library."""
    return _side_source_hash(CSRC_FEAT, FEAT_SOURCES)


def explain_source_hash():
    """source_hash() of the explanation library."""
    return _side_source_hash(CSRC_EXPLAIN, EXPLAIN_SOURCES)


def _stale(lib, digest):
    if not os.path.exists(lib):
        return True
    try:
        with open(lib + ".srchash") as fh:
            return fh.read().strip() != digest()
    except IOError:
        return True


def needs_build():
    """Stale unless the hash recorded next to the .so equals the hash of the sources as they are now (mtimes are meaningless after a
    checkout or a snapshot push; a .so shipped without its hash file is rebuilt where a compiler exists and trusted where none does).
    True if any of the libraries is stale."""
    return (_stale(LIB, source_hash) or _stale(EXT_LIB, ext_source_hash) or _stale(OPT_LIB, opt_source_hash) or _stale(TRAIN_LIB, train_source_hash) or
            _stale(INFER_LIB, infer_source_hash) or _stale(FEAT_LIB, feat_source_hash) or _stale(EXPLAIN_LIB, explain_source_hash))


def build(force=False, verbose=True):
    """Compile every HIP source for gfx950 and link the seven shared libraries, each only if it is stale (no GPU needed)."""
    os.makedirs(LIBDIR, exist_ok=True)
    if force or _stale(LIB, source_hash):
        _compile_and_link(LIB, CSRC, SOURCES, FLAGS + os.environ.get("URSO_VARIANT_FLAGS", "").split(), ("_" + VARIANT) if VARIANT else "", source_hash, verbose)
    if force or _stale(EXT_LIB, ext_source_hash):
        _compile_and_link(EXT_LIB, CSRC_EXT, EXT_SOURCES, FLAGS, "_ext", ext_source_hash, verbose)
    if force or _stale(OPT_LIB, opt_source_hash):
        _compile_and_link(OPT_LIB, CSRC_OPT, OPT_SOURCES, FLAGS, "_opt", opt_source_hash, verbose)
    if force or _stale(TRAIN_LIB, train_source_hash):
        _compile_and_link(TRAIN_LIB, CSRC_TRAIN, TRAIN_SOURCES, FLAGS, "_train", train_source_hash, verbose)
    if force or _stale(INFER_LIB, infer_source_hash):
        _compile_and_link(INFER_LIB, CSRC_INFER, INFER_SOURCES, FLAGS, "_infer", infer_source_hash, verbose)
    if force or _stale(FEAT_LIB, feat_source_hash):
        _compile_and_link(FEAT_LIB, CSRC_FEAT, FEAT_SOURCES, FLAGS, "_feat", feat_source_hash, verbose)
    if force or _stale(EXPLAIN_LIB, explain_source_hash):
        _compile_and_link(EXPLAIN_LIB, CSRC_EXPLAIN, EXPLAIN_SOURCES, FLAGS, "_explain", explain_source_hash, verbose)
    return LIB


def _compile_and_link(lib, srcdir, sources, flags, tag, digest, verbose):
    objs = []
    procs = []
    for s in sources:
        o = os.path.join(LIBDIR, s.replace(".hip", tag + ".o"))
        objs.append(o)
        cmd = [_hipcc()] + flags + ["-c", os.path.join(srcdir, s), "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for s, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError("hipcc failed on %s:\n%s" % (s, out.decode(errors="replace")))
        if verbose and out.strip():
            print(out.decode(errors="replace"))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(lib + ".srchash", "w") as fh:
        fh.write(digest() + "\n")


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print("built", LIB, EXT_LIB, OPT_LIB, TRAIN_LIB, INFER_LIB, FEAT_LIB, EXPLAIN_LIB)
