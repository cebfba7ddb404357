"""The certified walk's one-exit loop (cert_walk, csrc/vrt_cert.h) on inputs that leave the loop every
way it can be left. CPU part: the model of the walk (scripts/certsim.c, which tallies the way out
of each primary and shadow walk) over the inputs below must reach each class with at least one
pixel: a hit with no near-edge flag, the shadow walk's one-flag hit, unsure at an event with flags,
the corner block (left unsure, and passed), the length-limited miss and its tie case, and the miss
by leaving the volume; and its certified outcomes must agree with the exact walk's. GPU part: each
input through every certified path (certified mode 1; certified trees off and forced; the exact
path in lane and deferred), as a whole frame, as the 16-row block bands of a 2-way split and as a
two-frame batch, equal to the exact STATS instance byte for byte.
Frames of 64x48 and 96x64; the built scenes at N = 16 and 32 and the volumes of
tests/adversarial_volumes.py. max_ray_length 9 makes walks end by the length test."""
import ctypes as C

import numpy as np
import pytest

import voxelraytracer_amd as vrt
from adversarial_volumes import camera_poses, scene_volume
from harness import band, batch, certified_mode, load_certsim, reset_modes
from voxelraytracer_amd.tiles import block_band_spec

# name, volume (a built scene or adversarial/<name>), N, camera keywords, frame, max_ray_length (None: default)
LATTICE_DOWN = dict(pos=(1.0, -2.0, 3.0), rot=(-45.0, 0.0, 0.0))
INPUTS = [(f"{s}{n}_{w}x{h}", s, n, {}, (w, h), None)
          for s in ("refraction", "terrain", "glass_cube") for n, (w, h) in ((16, (96, 64)), (32, (64, 48)))]
INPUTS += [
    ("terrain32_lattice_point", "terrain", 32, "c1", (64, 48), None),                # corner blocks: unsure and passed
    ("bytes32_lattice_point", "adversarial/bytes", 32, "c1", (64, 48), None),       # events with flags, corner blocks
    ("bytes32_lattice_point_len9", "adversarial/bytes", 32, "c1", (64, 48), 9.0),   # length-limited misses, ties among them
    ("bytes32_diagonal_len9", "adversarial/bytes", 32, "c2", (64, 48), 9.0),        # shadow walks' length ties
    ("shell32_default", "adversarial/shell", 32, "c0", (64, 48), None),             # the shadow walk's one-flag hit
    ("shell16_lattice_down", "adversarial/shell", 16, LATTICE_DOWN, (96, 64), None),  # the same, three pixels
    ("bytes32_default", "adversarial/bytes", 32, "c0", (64, 48), None),
]
IDS = [i[0] for i in INPUTS]


def camera_of(n, cam, w, h):
    kw = camera_poses(n)[cam] if isinstance(cam, str) else cam
    return vrt.make_camera(w, h, **kw)


def params_of(max_len, **kw):
    if max_len is not None:
        kw["max_ray_length"] = max_len
    return vrt.default_params(4, 4, **kw)


# the model's tally slots (scripts/certsim.c, enum X_*)
X = {name: i for i, name in enumerate(
    "none hit hit_one_flag event_flags event_len corner ahead behind len_miss len_tie outside cap corner_passed".split())}


@pytest.fixture(scope="module")
def certsim(built):
    return load_certsim()


def model(L, vox, n, cam, p):
    """(cs_run's counts, exits[kind][class]) of one input."""
    vox = np.ascontiguousarray(vox, np.uint8)
    L.cs_build(vox.ctypes.data, n, 64)
    sun = np.array(p.sun_dir[:], np.float32)
    inv = np.array(cam.inv_pv[:], np.float32)
    o = np.zeros(32, np.float64)
    L.cs_exits_reset()
    L.cs_run(inv.ctypes.data, cam.width, cam.height, sun.ctypes.data, C.c_float(p.max_ray_length), 1.0,
             C.c_float(1.0 / 64), o.ctypes.data)
    x = np.zeros(2 * len(X), np.float64)
    assert L.cs_exits(x.ctypes.data) == len(X)
    return o, x.reshape(2, len(X))


def test_inputs_reach_every_way_out_of_the_loop(certsim):
    """No GPU: the model's walks over INPUTS. Each class is reached by at least one pixel, and no
    certified outcome of the model disagrees with the exact walk beside it."""
    total = np.zeros((2, len(X)))
    for name, scene, n, cam, (w, h), max_len in INPUTS:
        o, x = model(certsim, scene_volume(scene, n), n, camera_of(n, cam, w, h), params_of(max_len))
        assert o[6] == 0 and o[18] == 0, (name, o[6], o[18])
        total += x
    both = total.sum(axis=0)
    print({k: (int(total[0, i]), int(total[1, i])) for k, i in X.items()})
    for k in ("hit", "event_flags", "corner", "corner_passed", "len_miss", "len_tie", "outside"):
        assert both[X[k]] >= 1, (k, both)
    assert total[1, X["hit_one_flag"]] >= 1, total[1]          # a shadow walk's outcome only
    assert total[0, X["hit_one_flag"]] == 0, total[0]
    for kind in (0, 1):                                          # both walks: hit, leave, end by length
        for k in ("hit", "outside", "len_miss", "len_tie"):
            assert total[kind, X[k]] >= 1, (kind, k, total[kind])
    assert both[X["cap"]] == 0 and both[X["none"]] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,scene,n,cam,shape,max_len", INPUTS, ids=IDS)
def test_every_certified_path_equals_the_exact_instance(built, certsim, name, scene, n, cam, shape, max_len):
    w, h = shape
    vox = scene_volume(scene, n)
    cams = [camera_of(n, cam, w, h), camera_of(n, cam, w, h)]
    ps = [params_of(max_len, time=1.0), params_of(max_len, time=2.0)]
    bands = [(0, h, 1, 1)] + [block_band_spec(k, 2, h, 16) + (16,) for k in range(2)]
    # the share of pixels the reference alone says the plain certified pass defers: the model's
    # unsure pixels plus the exact instance's glass primaries (tests/test_gpu_cert_lean.py's bound;
    # with forced trees glass primaries stay, and glass_cube 16 is judged by that share, as there)
    o, _ = model(certsim, vox, n, cams[0], ps[0])
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        _, hits, _ = r.render(cams[0], ps[0])
        vi = hits["voxel_index"].reshape(-1)
        glass = int(np.count_nonzero(np.asarray(vox)[np.maximum(vi, 0)][vi >= 0] == 2))
        plain, trees = (o[19] + glass) / (w * h), o[19] / (w * h)
        print(f"{name}: deferred share (model) plain {plain:.3f}, trees {trees:.3f}")
        assert (trees if scene == "glass_cube" else plain) < 0.5
        for row0, rows, step, block in bands:
            if rows == 0:
                continue
            reset_modes(r)
            ref = [band(r, cams[f], ps[f], row0, rows, step, block, counters=True) for f in range(2)]
            for trees_mode in (0, 2):
                for exact_pass in (0, 2):
                    certified_mode(r, trees_mode, exact_pass)
                    for f in range(2):
                        got = band(r, cams[f], ps[f], row0, rows, step, block)
                        bad = np.argwhere(got != ref[f])
                        assert bad.size == 0, (row0, rows, block, trees_mode, exact_pass, f, bad[:5].tolist())
                    out = batch(r, cams, ps, row0, rows, step, block)
                    for f in range(2):
                        assert np.array_equal(out[f], ref[f]), ("batch", row0, rows, block, trees_mode, exact_pass, f)
