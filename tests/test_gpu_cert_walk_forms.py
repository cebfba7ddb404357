"""GPU: the certified walk's factored bound, flat jump test and one-rounding landing (vrt_cert.h
cert_walk; tests/test_cert_bound_forms.py holds the CPU restatement) through the certified pass with
the deferred exact pass forced, plain and with bounce trees, against the exact STATS instance, bit
for bit: the default camera; cameras in the cell layer next to each face of the volume, whose
walks start without a jump box (G <= 1: the flat test's no-jump case from the first iteration);
and lattice cameras with a direction component near zero (harness.LATTICE, straight down and
the axis views), where |1/d_b| B(u) dominates gam_b. glass_cube's trees walk from uncertain origins
(e0, ed, len0b != 0); the primary and exact-origin walks run the instance that adds no ed."""
import pytest

import numpy as np

import voxelraytracer_amd as vrt
from harness import LATTICE, band, certified_modes, reset_modes

pytestmark = pytest.mark.gpu

SCENES = [("refraction", 16), ("glass_cube", 32), ("terrain", 32)]
FRAMES = [(130, 70), (97, 65)]
ROTS = [(0.0, 0.0, 0.0), (-30.0, 45.0, 0.0)]


def face_layer(n):
    """Positions (relative to the volume's centre) in the cells next to each face."""
    e = n / 2.0
    out = []
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            q = [0.25, 0.5, -0.75]
            q[axis] = sgn * (e - 0.5)
            out.append(tuple(q))
    return out


def cameras(n):
    cams = [("default", {})]
    cams += [(f"face{i}_{j}", dict(pos=p, rot=r)) for i, p in enumerate(face_layer(n)) for j, r in enumerate(ROTS)]
    near_zero = list(LATTICE) + [((0.0, 0.0, 0.0), (-90.0, 0.0, 0.0)), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
                                 ((0.0, 0.0, 0.0), (0.0, 90.0, 0.0)), ((0.5, 0.5, 0.5), (0.0, 180.0, 0.0))]
    cams += [(f"lattice{i}", dict(pos=p, rot=r)) for i, (p, r) in enumerate(near_zero)]
    return cams


@pytest.fixture(scope="module", params=SCENES, ids=[f"{s}{n}" for s, n in SCENES])
def scene(built, request):
    name, n = request.param
    r = vrt.Renderer(0)
    r.upload_volume(vrt.build_scene(name, n), n)
    yield r, n
    r.close()


@pytest.mark.parametrize("w,h", FRAMES, ids=[f"{w}x{h}" for w, h in FRAMES])
def test_certified_pass_equals_exact_instance(scene, w, h):
    r, n = scene
    p = vrt.default_params(4, 4)
    try:
        for name, kw in cameras(n):
            cam = vrt.make_camera(w, h, **kw)
            reset_modes(r)
            ref = band(r, cam, p, counters=True)
            for trees in certified_modes(r):
                got = band(r, cam, p)
                bad = np.argwhere(got != ref)
                assert bad.size == 0, (name, trees, len(bad), bad[:5].tolist())
    finally:
        reset_modes(r)
