"""GPU: the shadow side of a primary hit in the certified pass (csrc/vrt_cert.h: cert_hit_record_primary,
cert_shade_hit<.., KAX>, cert_start_sun, the air cell's test and the prologue of the shadow walk) on scenes
built for that code. Every render mode (certified never / automatic / always, with and without certified trees,
the exact pass in lane and deferred) must give the exact STATS instance's RGBA8 frame byte for byte and its
float frame bit for bit.

Scenes, on 16^3 and 32^3 volumes, frames of at most 128x96:
 - a hollow room with a window in every wall and a pillar, seen from a corner with the sun behind the camera,
   once per sun octant: between them the views hit all six face orientations, lit and shadowed;
 - the room from cameras on integer and on half-integer positions (no launch-wide start cell / one);
 - a wall one cell in front of the camera: hits at the walk's first crossing, no jump before it;
 - a camera inside a solid voxel with a solid neighbour: the start cell is the one cell before a hit that the
   primary walk has not sampled, and the air cell's test must still defer those pixels;
 - a sun nearly parallel to two of the room's faces;
 - a short max_ray_length: the shadow's length limit ends walks;
 - a sun with a zero component: the generic lit term, and every lit hit deferred (KArgs::sun_ok == 0);
 - one textured frame (the reference atlas) and one frame batch of two cameras.
So that a frame in which everything is deferred cannot hide a broken certified path, the CPU model of the
certified walks (scripts/certsim.c) must find a certified shadow walk for at least half of the hit pixels of
every scene that has one by design (it finds 0.69 to 1.00 of them: test_scene prints each figure; the model
has no air cell test, so for the camera in a solid voxel it reports every pixel, where a diagnostic build of
the library counts 3 904 of 6 144 certified and 2 240 stopped by that test). The
zero-component sun has none by design (the certified pass defers every lit hit there), and for it the model
must say so too: its share is asserted to be zero, the other side of the same branch."""
import ctypes as C
import functools

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from harness import (all_modes, assert_equal, band, batch, current_stream, float_bits, load_certsim, ref_atlas,
                     reset_modes, view_direction)

pytestmark = pytest.mark.gpu


# ---- volumes ---------------------------------------------------------------------------------------

def room(n):
    """One-voxel walls of stone and grass on all six faces, a square window in the middle of each, and a
    grass pillar off the centre."""
    v = np.zeros((n, n, n), np.uint8)   # [z][y][x]
    v[0], v[-1] = 1, 3
    v[:, 0], v[:, -1] = 3, 1
    v[:, :, 0], v[:, :, -1] = 1, 3
    a, b = n // 2 - n // 8, n // 2 + n // 8
    for face in (v[0], v[-1], v[:, 0], v[:, -1], v[:, :, 0], v[:, :, -1]):
        face[a:b, a:b] = 0
    v[n // 2 + 1:n // 2 + 3, 1:n // 2, n // 2 - 3:n // 2 - 1] = 3
    return np.ascontiguousarray(v.reshape(-1))


def cell_of(pos, n):
    return tuple(int(np.floor(c + n / 2)) for c in pos)


def wall_ahead(n, pos, rot):
    """A stone wall filling the layer right in front of the camera's cell along its view axis; nothing else,
    so the shadow rays, which leave the wall towards the sun behind the camera, end lit."""
    d = view_direction(vrt.make_camera(8, 8, pos=pos, rot=rot))
    ax = int(np.argmax(np.abs(d)))
    c = cell_of(pos, n)
    v = np.zeros((n, n, n), np.uint8)
    idx = [slice(None)] * 3
    idx[2 - ax] = c[ax] + (1 if d[ax] > 0 else -1)
    v[tuple(idx)] = 1
    return np.ascontiguousarray(v.reshape(-1))


def solid_start(n, pos, rot):
    """The camera's cell solid, its +x neighbour solid too (pixels whose first crossing is +x hit it from the
    start cell), and a wall a few cells ahead for the other pixels."""
    d = view_direction(vrt.make_camera(8, 8, pos=pos, rot=rot))
    ax = int(np.argmax(np.abs(d)))
    assert ax == 2
    c = cell_of(pos, n)
    v = np.zeros((n, n, n), np.uint8)
    v[c[2] + (4 if d[2] > 0 else -4)] = 3
    v[c[2], c[1], c[0]] = 1
    v[c[2], c[1], c[0] + 1] = 1
    return np.ascontiguousarray(v.reshape(-1))


# ---- scenes ----------------------------------------------------------------------------------------

OCTANTS = [(x, y, z) for x in (1, -1) for y in (1, -1) for z in (1, -1)]
CORNER_ROTS = [(p, y, 0.0) for p in (-30.0, 30.0) for y in (45.0, 135.0, 225.0, 315.0)]


def corner_view(sun, w=8, h=8):
    """The corner view that looks most nearly away from the sun: the walls it sees face the sun."""
    s = np.array(sun, np.float64) / np.linalg.norm(sun)
    return min(CORNER_ROTS, key=lambda r: float(view_direction(vrt.make_camera(w, h, pos=(0.3, 0.2, 0.1), rot=r)) @ s))


def scenes():
    out = []
    for o in OCTANTS:   # the room, one view per sun octant
        sun = (0.45 * o[0], 0.7 * o[1], 0.55 * o[2])
        tag = "".join("+" if s > 0 else "-" for s in o)
        n = 16 if o[0] > 0 else 32
        out.append(dict(id=f"room{n}_sun{tag}", n=n, vox=room(n), size=(96, 64), sun=sun,
                        cams=[dict(pos=(0.3, 0.2, 0.1), rot=corner_view(sun))]))
    sun = (-0.45, 0.7, -0.55)
    out.append(dict(id="room16_integer_camera", n=16, vox=room(16), size=(65, 47), sun=sun,
                    cams=[dict(pos=(1.0, -1.0, 2.0), rot=corner_view(sun))]))
    out.append(dict(id="room32_half_integer_camera", n=32, vox=room(32), size=(128, 96), sun=sun,
                    cams=[dict(pos=(0.5, -1.5, 2.5), rot=corner_view(sun))]))
    pos, rot = (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)
    d = view_direction(vrt.make_camera(8, 8, pos=pos, rot=rot))
    back = tuple(float(x) for x in (-0.6 * np.sign(d) + np.array([0.3, 0.45, 0.0])))   # the sun behind the camera
    out.append(dict(id="wall_one_cell_ahead16", n=16, vox=wall_ahead(16, pos, rot), size=(96, 64), sun=back,
                    cams=[dict(pos=pos, rot=rot)]))
    # (the sun on the -x side: the solid neighbour's face, normal -x, is lit, so its pixels pass the back-face
    # test and the shadow's start and reach the air cell's test, which finds the solid start cell)
    pos2, side = (0.8, 0.5, 0.5), (-back[0], back[1], back[2])
    out.append(dict(id="camera_in_solid_voxel16", n=16, vox=solid_start(16, pos2, rot), size=(96, 64), sun=side,
                    cams=[dict(pos=pos2, rot=rot)]))
    sun = (2e-3, 0.8, -1e-3)
    out.append(dict(id="room16_sun_near_parallel", n=16, vox=room(16), size=(96, 64), sun=sun,
                    cams=[dict(pos=(0.3, 2.2, 0.1), rot=(-60.0, 45.0, 0.0))]))
    sun = (-0.45, 0.7, -0.55)
    out.append(dict(id="room32_short_max_len", n=32, vox=room(32), size=(96, 64), sun=sun, max_ray_length=24.0,
                    cams=[dict(pos=(0.3, 0.2, 0.1), rot=corner_view(sun))]))
    sun = (0.0, 0.8, -0.6)
    out.append(dict(id="room16_sun_zero_component", n=16, vox=room(16), size=(96, 64), sun=sun, none_by_design=True,
                    cams=[dict(pos=(0.3, 0.2, 0.1), rot=corner_view(sun))]))
    sun = (0.45, 0.7, 0.55)
    out.append(dict(id="room16_textured", n=16, vox=room(16), size=(96, 64), sun=sun, textured=True,
                    cams=[dict(pos=(0.3, 0.2, 0.1), rot=corner_view(sun))]))
    out.append(dict(id="room32_frame_batch", n=32, vox=room(32), size=(96, 64), sun=sun,
                    cams=[dict(pos=(0.3, 0.2, 0.1), rot=corner_view(sun)), dict(pos=(-2.3, 1.2, 3.1), rot=corner_view(sun))]))
    return out


# (the scenes need the built library for their cameras: they are made inside the test, by id)
SCENE_IDS = ([f"room{16 if o[0] > 0 else 32}_sun{''.join('+' if s > 0 else '-' for s in o)}" for o in OCTANTS] +
             ["room16_integer_camera", "room32_half_integer_camera", "wall_one_cell_ahead16", "camera_in_solid_voxel16",
              "room16_sun_near_parallel", "room32_short_max_len", "room16_sun_zero_component", "room16_textured",
              "room32_frame_batch"])


@functools.lru_cache(maxsize=None)
def scene_table():
    table = {s["id"]: s for s in scenes()}
    assert list(table) == SCENE_IDS, list(table)
    return table


def scene_params(sc, time=1.0):
    kw = dict(sun_dir=sc["sun"], time=time)
    if "max_ray_length" in sc:
        kw["max_ray_length"] = sc["max_ray_length"]
    p = vrt.default_params(4, 4, **kw)
    return vrt.textured_params(p, ref_atlas(), 128) if sc.get("textured") else p


def model_share(certsim, sc, cam, p):
    """(certified shadow walks, hit pixels) of one camera by the CPU model: o[17] counts the shadow walks that
    end certified (blocked or lit), o[7] the certified primary hits and o[8] the exact walk's non-glass hits;
    the larger of the two is the number of hit pixels (these scenes hold no glass)."""
    w, h = sc["size"]
    certsim.cs_build(np.ascontiguousarray(sc["vox"], np.uint8).ctypes.data, sc["n"], 64)
    inv = np.array(cam.inv_pv[:], np.float32)
    sun = np.array(p.sun_dir[:], np.float32)
    o = np.zeros(32, np.float64)
    certsim.cs_run(inv.ctypes.data, w, h, sun.ctypes.data, C.c_float(p.max_ray_length), 1.0, C.c_float(1.0 / 64),
                   o.ctypes.data)
    return int(o[17]), int(max(o[7], o[8]))


def float_frame(r, cam, p, counters=False):
    import torch

    out = torch.zeros((cam.height, cam.width, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(len(vrt.COUNTER_NAMES), dtype=torch.int64, device="cuda")
    r.render_rows_async(cam, p, 0, cam.height, 1, out.data_ptr(), 0, cnt.data_ptr() if counters else 0,
                        current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def certsim(built):
    return load_certsim()


@pytest.mark.parametrize("sid", SCENE_IDS)
def test_scene(built, certsim, sid):
    sc = scene_table()[sid]
    w, h = sc["size"]
    cams = [vrt.make_camera(w, h, **kw) for kw in sc["cams"]]
    ps = [scene_params(sc, time=float(f + 1)) for f in range(len(cams))]
    for cam, p in zip(cams, ps):
        walks, hits = model_share(certsim, sc, cam, p)
        print(f"{sc['id']}: model: {walks} certified shadow walks of {hits} hit pixels ({w}x{h})")
        assert hits >= w * h // 4, (sc["id"], hits)
        if sc.get("none_by_design"):
            assert walks == 0, (sc["id"], walks)
        else:
            assert 2 * walks >= hits, (sc["id"], walks, hits)
    with vrt.Renderer(0) as r:
        r.upload_volume(sc["vox"], sc["n"])
        reset_modes(r)
        ref8 = [band(r, cam, p, counters=True) for cam, p in zip(cams, ps)]
        ref32 = [float_frame(r, cam, p, counters=True) for cam, p in zip(cams, ps)]
        for mode in all_modes(r):
            for f, (cam, p) in enumerate(zip(cams, ps)):
                assert_equal(band(r, cam, p), ref8[f], (sc["id"], "rgba8", mode, f))
                assert_equal(float_bits(float_frame(r, cam, p)), float_bits(ref32[f]), (sc["id"], "float", mode, f))
            if len(cams) > 1:
                got = batch(r, cams, ps)
                for f in range(len(cams)):
                    assert_equal(got[f], ref8[f], (sc["id"], "batch", mode, f))
