"""The ID and depth pass on the CPU: vrt_pixel_id's layout and its ctypes / NumPy mirrors, the three
entry points in the header, the mirror and the built library, and the host helpers (hit_normal,
hit_cell, adjacent_cell) on the new records. No GPU."""
import ctypes as C
import os

import numpy as np

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vrt_render_ids_async", "vrt_render_ids", "vrt_ids_deferred")


def test_pixel_id_layout():
    assert C.sizeof(abi.PixelId) == 8
    assert (abi.PixelId.voxel_index.offset, abi.PixelId.face.offset) == (0, 4)
    d = np.dtype(abi.PIXEL_ID_DTYPE)
    assert d.itemsize == 8
    assert [(name, d.fields[name][1], d.fields[name][0].str) for name, _ in abi.PIXEL_ID_DTYPE] == \
        [("voxel_index", 0, "<i4"), ("face", 4, "<u4")]
    # the two mirrors read the same bytes
    rec = np.zeros(1, abi.PIXEL_ID_DTYPE)
    rec["voxel_index"], rec["face"] = -1, 0x0302
    c = abi.PixelId.from_buffer_copy(rec.tobytes())
    assert c.voxel_index == -1 and c.face == 0x0302
    # vrt_ray_hit's fields of the same names, with the same types
    hit = np.dtype(abi.RAY_HIT_DTYPE)
    assert all(hit.fields[name][0] == d.fields[name][0] for name in ("voxel_index", "face"))
    assert vrt.PIXEL_ID_DTYPE is abi.PIXEL_ID_DTYPE and vrt.PixelId is abi.PixelId


def test_entry_points_in_header_mirror_and_library(built):
    header = open(os.path.join(ROOT, "include", "vrt.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert name in abi.SIGNATURES, name
        assert abi.ADDED_IN[name] == 16
        assert hasattr(lib, name), name
    assert "typedef struct { int32_t voxel_index; uint32_t face; } vrt_pixel_id;" in header
    assert "#define VRT_ABI_VERSION 15" in header   # added within v15
    assert len(abi.SIGNATURES["vrt_render_ids_async"][1]) == 9
    assert len(abi.SIGNATURES["vrt_render_ids"][1]) == 5
    assert len(abi.SIGNATURES["vrt_ids_deferred"][1]) == 3


def test_renderer_has_the_host_methods():
    for name in ("render_ids", "render_ids_async", "ids_deferred"):
        assert callable(getattr(vrt.Renderer, name))


def test_hit_helpers_accept_pixel_ids():
    """The helpers read voxel_index and face only, so a frame of vrt_pixel_id records decodes like the
    same fields of vrt_ray_hit records."""
    n = 16
    ids = np.zeros((2, 3), abi.PIXEL_ID_DTYPE)
    ids["voxel_index"] = [[5 + 3 * n + 15 * n * n, -1, 0], [7, 8 + n, 9 + 2 * n * n]]
    ids["face"] = [[2 | 4 | (3 << 8), 0, 2 | 4 | (1 << 8)], [0 | (2 << 8), 1 | 4 | (1 << 8), 1 | (1 << 8)]]
    hits = np.zeros(6, abi.RAY_HIT_DTYPE)
    hits["voxel_index"], hits["face"] = ids["voxel_index"].reshape(-1), ids["face"].reshape(-1)
    assert np.array_equal(vrt.hit_normal(ids), vrt.hit_normal(hits))
    assert vrt.hit_normal(ids).tolist() == [[0, 0, -1], [0, 0, 0], [0, 0, -1], [1, 0, 0], [0, -1, 0], [0, 1, 0]]
    for got, want in zip(vrt.hit_cell(ids, n), vrt.hit_cell(hits, n)):
        assert np.array_equal(got, want)
    i, j, k = vrt.hit_cell(ids, n)
    assert list(zip(i.tolist(), j.tolist(), k.tolist())) == [(5, 3, 15), (-1, -1, -1), (0, 0, 0), (7, 0, 0),
                                                             (8, 1, 0), (9, 0, 2)]
    ai, aj, ak = vrt.adjacent_cell(ids, n)
    assert list(zip(ai.tolist(), aj.tolist(), ak.tolist())) == [(5, 3, 14), (-1, -1, -1), (0, 0, -1), (8, 0, 0),
                                                                (8, 0, 0), (9, 1, 2)]
