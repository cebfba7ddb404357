"""The certified ID kernel's switch on the CPU: vrt_set_ids_certified and vrt_ids_certified in the header,
the ctypes mirror and the built library (added within v15), and the Renderer's methods. No GPU."""
import ctypes as C
import os

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"vrt_set_ids_certified": 2, "vrt_ids_certified": 1}


def test_entry_points_in_header_mirror_and_library(built):
    header = open(os.path.join(ROOT, "include", "vrt.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name, arity in ENTRY_POINTS.items():
        assert f"int {name}(" in header, name
        assert name in abi.SIGNATURES, name
        restype, argtypes = abi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == arity, name
        assert abi.ADDED_IN[name] == 16, name
        assert hasattr(lib, name), name
    assert abi.SIGNATURES["vrt_set_ids_certified"][1] == [C.c_void_p, C.c_int32]
    assert "int vrt_set_ids_certified(vrt_ctx* ctx, int32_t mode);" in header
    assert "int vrt_ids_certified(const vrt_ctx* ctx);" in header


def test_added_within_v15(built):
    header = open(os.path.join(ROOT, "include", "vrt.h")).read()
    assert "#define VRT_ABI_VERSION 15" in header
    lib = C.CDLL(abi.LIB_PATH)
    lib.vrt_abi_version.restype = C.c_int
    assert lib.vrt_abi_version() == 15


def test_null_context_is_invalid(built):
    """Neither entry point touches the device for a null context."""
    lib = C.CDLL(abi.LIB_PATH)
    for name, (res, args) in ((k, abi.SIGNATURES[k]) for k in ENTRY_POINTS):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    assert lib.vrt_set_ids_certified(None, 1) == abi.VRT_ERR_INVALID
    assert lib.vrt_ids_certified(None) == abi.VRT_ERR_INVALID


def test_renderer_has_the_host_methods():
    for name in ("set_ids_certified", "ids_certified"):
        assert callable(getattr(vrt.Renderer, name))
    assert "no certified ID kernel" not in vrt.Renderer.ids_deferred.__doc__
