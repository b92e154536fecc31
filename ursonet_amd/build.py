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
# The libraries behind the main one, in the order they were added: name -> sources.  Everything else follows from the name: the source
# directory csrc_<name>, lib/liburso_<name>.so, the header include/ursonet_<name>.h and the object-file tag _<name>.  Same flags, no
# variant; each calls into the main library (error text, launch profiler), which the loader resolves when it loads one behind it
# (ursonet_amd/hip.py: side_lib).  A new library is a new row here and a row of signatures in hip.SIDE_SIGS.
SIDE_SOURCES = {
    "ext": ["pose_fuse.hip", "loss_weights.hip", "weight_ema.hip", "grad_accum.hip", "lars.hip"],   # entry points added after liburso_hip.so's surface was frozen
    "opt": ["lamb.hip"],                                                                             # optimizers, after liburso_ext.so's was frozen too
    "train": ["sam.hip", "bn_recal.hip", "swa.hip", "ensemble.hip", "calibrate.hip"],                # training features; its own surface stays open
    "infer": ["conformal.hip"],                                                                      # conformal bounds (ursonet_amd/conformal.py)
    "feat": ["feat.hip"],                                                                            # feature-space statistics (ursonet_amd/domain.py)
    "explain": ["explain.hip"],                                                                      # occlusion-sensitivity maps (ursonet_amd/explain.py)
}
SIDE_LIBS = {name: os.path.join(LIBDIR, "liburso_%s.so" % name) for name in SIDE_SOURCES}           # patchable one library at a time
__doc__ = ("Builds liburso_hip.so and, behind it, %s (gfx950) in-tree with hipcc.  `python -m ursonet_amd.build`."
           % ", ".join("liburso_%s.so" % name for name in SIDE_SOURCES))


def side_srcdir(name):
    return os.path.join(HERE, "csrc_" + name)


def side_header(name):
    return os.path.join(HERE, "..", "include", "ursonet_%s.h" % name)


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


def side_source_hash(name):
    """source_hash() of a library behind the main one: every file of its source directory, the headers of csrc/ it may include, the public
    headers, the compile flags and the compiler's version string."""
    import hashlib
    h = hashlib.sha256()
    srcdir, inc = side_srcdir(name), os.path.join(HERE, "..", "include")
    files = (sorted(os.path.join(srcdir, f) for f in os.listdir(srcdir)) + sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) +
             sorted(os.path.join(inc, f) for f in os.listdir(inc) if f.endswith(".h")))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
        h.update(b"\0")
    h.update(" ".join(FLAGS + SIDE_SOURCES[name]).encode())
    _hash_compiler(h)
    return h.hexdigest()


def _stale(lib, digest):
    if not os.path.exists(lib):
        return True
    try:
        with open(lib + ".srchash") as fh:
            return fh.read().strip() != digest()
    except IOError:
        return True


def side_stale(name):
    return _stale(SIDE_LIBS[name], lambda: side_source_hash(name))


def needs_build():
    """Stale unless the hash recorded next to the .so equals the hash of the sources as they are now (mtimes are meaningless after a
    checkout or a snapshot push; a .so shipped without its hash file is rebuilt where a compiler exists and trusted where none does).
    True if any of the libraries is stale."""
    return _stale(LIB, source_hash) or any(side_stale(name) for name in SIDE_SOURCES)


def build(force=False, verbose=True):
    """Compile every HIP source for gfx950 and link the main library and every library of SIDE_SOURCES, each only if it is stale (no GPU
    needed)."""
    os.makedirs(LIBDIR, exist_ok=True)
    if force or _stale(LIB, source_hash):
        _compile_and_link(LIB, CSRC, SOURCES, FLAGS + os.environ.get("URSO_VARIANT_FLAGS", "").split(), ("_" + VARIANT) if VARIANT else "", source_hash, verbose)
    for name, sources in SIDE_SOURCES.items():
        if force or side_stale(name):
            _compile_and_link(SIDE_LIBS[name], side_srcdir(name), sources, FLAGS, "_" + name, lambda: side_source_hash(name), verbose)
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
    print("built", LIB, *SIDE_LIBS.values())
