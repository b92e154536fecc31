"""The libraries behind liburso_hip.so without a GPU, one case per row of build.SIDE_SOURCES: the surface (header = bindings = nm, the
sources on disk, no name shared with another library) and the build's staleness check (tests/libsurface.py).  Loading a side library
initialises no GPU."""
import pytest

import libsurface
from ursonet_amd.build import SIDE_SOURCES


@pytest.mark.parametrize("name", list(SIDE_SOURCES))
def test_header_bindings_library_and_sources_agree(name):
    libsurface.check_surface(name)


@pytest.mark.parametrize("name", list(SIDE_SOURCES))
def test_the_build_knows_the_library(name, monkeypatch, tmp_path):
    libsurface.check_staleness(name, monkeypatch, tmp_path)
