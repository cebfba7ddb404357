"""Ray queries on the CPU: the records' layout (vrt_ray, vrt_ray_hit and their ctypes / NumPy
mirrors), the three entry points in the header, the mirror and the built library, make_rays' packing
and the host helpers that decode a record (hit_normal, hit_cell, adjacent_cell). No GPU."""
import ctypes as C
import os
import struct

import numpy as np

import voxelraytracer_amd as vrt
from voxelraytracer_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("vrt_cast_rays_async", "vrt_cast_rays", "vrt_pick_pixels")


def test_record_sizes():
    assert C.sizeof(abi.Ray) == C.sizeof(abi.RayHit) == 32
    assert np.dtype(abi.RAY_DTYPE).itemsize == np.dtype(abi.RAY_HIT_DTYPE).itemsize == 32
    assert vrt.RAY_DTYPE is abi.RAY_DTYPE and vrt.RAY_HIT_DTYPE is abi.RAY_HIT_DTYPE


def test_ray_hit_starts_with_a_hit():
    assert abi.RAY_HIT_DTYPE[:4] == abi.HIT_DTYPE
    d = np.dtype(abi.RAY_HIT_DTYPE)
    assert [d.fields[name][1] for name, *_ in abi.RAY_HIT_DTYPE] == [0, 4, 8, 12, 16, 28]
    for (name, _), (cname, _) in zip(abi.Hit._fields_, abi.RayHit._fields_[:4]):
        assert name == cname and getattr(abi.Hit, name).offset == getattr(abi.RayHit, name).offset
    assert abi.RayHit.point.offset == 16 and abi.RayHit.face.offset == 28
    assert (abi.Ray.origin.offset, abi.Ray.max_length.offset, abi.Ray.dir.offset, abi.Ray.reserved.offset) == \
        (0, 12, 16, 28)


def test_entry_points_in_header_mirror_and_library(built):
    header = open(os.path.join(ROOT, "include", "vrt.h")).read()
    lib = C.CDLL(abi.LIB_PATH)
    for name in ENTRY_POINTS:
        assert f"int {name}(" in header, name
        assert name in abi.SIGNATURES, name
        assert abi.ADDED_IN[name] == 16
        assert hasattr(lib, name), name
    assert "#define VRT_RAY_FLAG_BLOCKED 8u" in header and abi.VRT_RAY_FLAG_BLOCKED == 8
    assert "VRT_CAST_NEAREST = 0, VRT_CAST_OCCLUSION = 1" in header
    assert abi.CAST_MODES == {"nearest": 0, "occlusion": 1}
    assert "#define VRT_ABI_VERSION 15" in header   # added within v15


def test_make_rays_packs_fields_at_their_offsets():
    origins = np.array([[1.5, -2.25, 3.0], [16.0, 8.5, 8.5]], np.float32)
    dirs = np.array([[0.0, -0.0, 1.0], [-1.0, 1e-30, 0.5]], np.float32)
    rays = vrt.make_rays(origins, dirs, [7.5, 100.0])
    assert rays.dtype == np.dtype(abi.RAY_DTYPE) and rays.shape == (2,)
    raw = rays.tobytes()
    for i in range(2):
        rec = raw[32 * i:32 * (i + 1)]
        assert rec[0:12] == origins[i].tobytes()
        assert rec[12:16] == struct.pack("<f", [7.5, 100.0][i])
        assert rec[16:28] == dirs[i].tobytes()       # bit patterns kept: -0.0 stays -0.0
        assert rec[28:32] == b"\0\0\0\0"
    # one max_length for all rays, and its default
    assert np.all(vrt.make_rays(origins, dirs, 3.0)["max_length"] == np.float32(3.0))
    assert np.all(vrt.make_rays(origins, dirs)["max_length"] == np.float32(100.0))
    # the ctypes mirror reads the same bytes
    r0 = abi.Ray.from_buffer_copy(raw[:32])
    assert list(r0.origin) == [1.5, -2.25, 3.0] and r0.max_length == 7.5 and list(r0.dir) == [0.0, -0.0, 1.0]


def record(voxel_index, axis=0, negative=False, byte=1):
    h = np.zeros(1, abi.RAY_HIT_DTYPE)
    h["voxel_index"] = voxel_index
    h["face"] = axis | (4 if negative else 0) | (byte << 8)
    return h


def test_hit_helpers_on_hand_built_records():
    n = 16
    cell = (5, 3, 15)   # on the volume's border in z
    idx = cell[0] + cell[1] * n + cell[2] * n * n
    recs, normals = [], []
    for axis in range(3):
        for negative in (False, True):
            recs.append(record(idx, axis, negative, byte=3))
            nrm = [0, 0, 0]
            nrm[axis] = -1 if negative else 1
            normals.append(nrm)
    recs.append(record(-1))            # a miss (a miss's face is 0)
    recs.append(record(0, 2, True))    # cell (0, 0, 0), face -z: the neighbour is outside the volume
    hits = np.concatenate(recs)
    nrm = vrt.hit_normal(hits)
    assert nrm.dtype == np.int8 and nrm.shape == (len(hits), 3)
    assert nrm.tolist() == normals + [[0, 0, 0], [0, 0, -1]]
    i, j, k = vrt.hit_cell(hits, n)
    assert i.tolist() == [5] * 6 + [-1, 0] and j.tolist() == [3] * 6 + [-1, 0] and k.tolist() == [15] * 6 + [-1, 0]
    ai, aj, ak = vrt.adjacent_cell(hits, n)
    assert list(zip(ai.tolist(), aj.tolist(), ak.tolist())) == [
        (6, 3, 15), (4, 3, 15), (5, 4, 15), (5, 2, 15), (5, 3, 16), (5, 3, 14), (-1, -1, -1), (0, 0, -1)]
    # the voxel byte rides in bits 8-15 and does not disturb the decode
    assert ((hits["face"] >> 8) & 0xFF).tolist() == [3] * 6 + [1, 1]
