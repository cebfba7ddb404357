"""The ID-guided spatial filter on the CPU: its three entry points in the header, the ctypes mirror and the built
library, the constants in the header and the binding, and the host methods. It is added within ABI v15. No GPU."""
import ctypes as C
import os
import re

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"vrt_spatial_filter_async": 15, "vrt_spatial_filter": 10, "vrt_set_reprojected_spatial": 5}


def test_entry_points_in_header_mirror_and_library(built):
    header = open(os.path.join(ROOT, "include", "vrt.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        assert f"int {name}(" in header, name
        assert name in abi.SIGNATURES, name
        assert abi.ADDED_IN[name] == 16
        assert hasattr(lib, name), name
        restype, argtypes = abi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == nargs, name
        # the header's own argument count
        decl = re.search(r"int %s\((.*?)\);" % name, header, flags=re.S).group(1)
        assert decl.count(",") + 1 == nargs, (name, decl)
    assert "#define VRT_ABI_VERSION 15" in header   # added within v15
    assert vrt.lib().vrt_abi_version() == 15


def test_constants_in_header_and_binding():
    header = open(os.path.join(ROOT, "include", "vrt.h")).read()
    assert "enum { VRT_GUIDE_FACE = 0, VRT_GUIDE_PLANE = 1 };" in header
    assert "enum { VRT_SPATIAL_OFF = 0, VRT_SPATIAL_DISPLAY = 1, VRT_SPATIAL_FILL = 2 };" in header
    assert (vrt.GUIDE_FACE, vrt.GUIDE_PLANE) == (0, 1)
    assert (vrt.SPATIAL_OFF, vrt.SPATIAL_DISPLAY, vrt.SPATIAL_FILL) == (0, 1, 2)
    for name in ("GUIDE_FACE", "GUIDE_PLANE", "SPATIAL_OFF", "SPATIAL_DISPLAY", "SPATIAL_FILL"):
        assert getattr(vrt, name) == getattr(abi, name)


def test_renderer_has_the_host_methods():
    for name in ("spatial_filter_async", "spatial_filter", "set_reprojected_spatial"):
        assert callable(getattr(vrt.Renderer, name))


def test_null_context_is_refused(built):
    L = vrt.lib()
    assert L.vrt_spatial_filter_async(None, 4, 4, 4, 1, 0, 765, 0, 4, None, None, None, None, None, None) == abi.VRT_ERR_INVALID
    assert L.vrt_spatial_filter(None, 4, 4, 3, 0, 765, None, None, None, None) == abi.VRT_ERR_INVALID
    assert L.vrt_set_reprojected_spatial(None, 0, 3, 0, 765) == abi.VRT_ERR_INVALID
