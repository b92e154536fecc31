"""What every library behind liburso_hip.so (ursonet_amd/build.py: SIDE_SOURCES) is checked for, whatever it holds: its surface and its
place in the build.  tests/test_side_libs_cpu.py runs both checks once per library; a feature's own test file keeps what is about the
feature (its names, macros, struct layouts, the C99 compile of its header, its argument checks) and takes header_symbols / defined from here."""
import os
import re
import subprocess

import pytest


def header_symbols(header):
    """(the urso_* functions a header declares, its text without comments)."""
    txt = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return set(re.findall(r"\b(urso_[a-z0-9_]+)\s*\(", txt)), txt


def defined(path):
    """The urso_* functions a shared library exports."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (urso_\w+)$", out, re.M))


def check_surface(name):
    """Header = bindings = nm, the loader binds every name, the source directory holds exactly the table's sources, and no other library
    (the main one and its loss-scaling extension included) exports or binds one of the names."""
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    names = header_symbols(build.side_header(name))[0]
    assert names and names == set(hip.SIDE_SYMBOLS[name]) == defined(build.SIDE_LIBS[name])
    lib = hip.side_lib(name)                                                 # loads and binds: a missing symbol raises
    assert all(hasattr(lib, nm) for nm in names)
    assert sorted(os.listdir(build.side_srcdir(name))) == sorted(build.SIDE_SOURCES[name])
    assert os.path.basename(build.SIDE_LIBS[name]) == "liburso_%s.so" % name
    assert list(hip.SIDE_SIGS) == list(build.SIDE_SOURCES)
    others = [(hip.LIB_PATH, hip.EXPORTED_SYMBOLS + hip.LOSS_SCALE_SYMBOLS)]
    others += [(build.SIDE_LIBS[other], hip.SIDE_SYMBOLS[other]) for other in build.SIDE_SOURCES if other != name]
    for path, table in others:
        assert names.isdisjoint(defined(path)) and names.isdisjoint(table), path


def check_staleness(name, monkeypatch, tmp_path):
    """The stamp next to the built library is the hash of its sources, the build is fresh as built, and with that one library missing the
    build is stale and the loader raises."""
    import ursonet_amd.hip as hip
    from ursonet_amd import build
    with open(build.SIDE_LIBS[name] + ".srchash") as fh:
        assert fh.read().strip() == build.side_source_hash(name)             # as built: the stamp is the hash of the sources
    assert not build.needs_build()
    assert "-ffp-contract=off" in build.FLAGS
    monkeypatch.setitem(build.SIDE_LIBS, name, str(tmp_path / ("liburso_%s.so" % name)))
    assert build.side_stale(name) and build.needs_build()                    # a missing library makes the build stale
    assert not any(build.side_stale(other) for other in build.SIDE_SOURCES if other != name)
    monkeypatch.delitem(hip._side, name, raising=False)
    with pytest.raises(ImportError, match=r"liburso_%s\.so not found at .* build it with `python -m ursonet_amd\.build`" % name):
        hip.side_lib(name)
