"""The once-per-pixel code around the certified pass's two walks (csrc/vrt_cert.h: cert_pixel's merged
start predicate and the start it hands cert_walk, cert_shade_hit's axis-normal lit term, the sun's
launch constants read late) on the starts and suns that reach its branches. The certified pass with the
deferred exact pass forced (set_exact_pass(2): the DEFER instances run at these frame sizes) must equal
the exact STATS instance byte for byte, as a plain launch, as a two-camera frame batch, with certified
trees forced on glass clutter, and textured with the reference atlas; the start cases' frames of the
16^3 volumes (the default sun, as in the existing oracle tests of these volumes) are also held to one
LSB of the C oracle under tests/test_gpu_temporal.py's contract.
Frames 64x48 and 33x33 (odd width, axis-aligned: the centre column has a zero direction component);
volumes 16^3 and 32^3: the six-face shell and the glass clutter of tests/adversarial_volumes.py.

test_start_cases[glass_clutter-32], camera outside_py at 33x33, is the case that found cert_continuation's
missing on-plane check: pixel (16, 18) differed in every certified mode until then."""
import os

import pytest

import oracle
import voxelraytracer_amd as vrt
from adversarial_volumes import volumes
from harness import assert_equal, band, batch, certified_mode, check_raw, ref_atlas, reset_modes, words_to_bytes

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)


def start_cameras(n):
    """Lattice cameras (integer and half-integer positions; axis, diagonal and straight-down views: ray
    origins on planes with rays moving down an axis), and one camera outside each face of the volume."""
    out = n / 2 + 3.0
    return {
        "lattice_axis": dict(pos=(0.0, 0.0, 0.0), rot=(0.0, 0.0, 0.0)),
        "lattice_axis_int": dict(pos=(1.0, 2.0, -3.0), rot=(0.0, 0.0, 0.0)),
        "lattice_half_diag": dict(pos=(-2.5, 0.5, 1.5), rot=(-35.26439, 45.0, 0.0)),
        "lattice_diag": dict(pos=(0.0, 0.0, 0.0), rot=(-45.0, -45.0, 0.0)),
        "lattice_yaw90": dict(pos=(3.0, -1.0, -2.0), rot=(0.0, 90.0, 0.0)),
        "lattice_down": dict(pos=(1.0, -2.0, 3.0), rot=(-45.0, 0.0, 0.0)),
        "straight_down": dict(pos=(0.5, 2.0, 0.5), rot=(-90.0, 0.0, 0.0)),
        "outside_pz": dict(pos=(0.0, 0.0, out), rot=(0.0, 0.0, 0.0)),
        "outside_nz": dict(pos=(0.5, 0.0, -out), rot=(0.0, 180.0, 0.0)),
        "outside_px": dict(pos=(out, 0.5, 0.5), rot=(0.0, 90.0, 0.0)),
        "outside_nx": dict(pos=(-out, 0.0, 0.5), rot=(0.0, -90.0, 0.0)),
        "outside_py": dict(pos=(0.0, out, 0.0), rot=(-90.0, 0.0, 0.0)),
        "outside_ny": dict(pos=(0.5, -out, 0.0), rot=(90.0, 0.0, 0.0)),
    }


# all eight octants, a zero component (the generic lit term behind the wave-uniform branch; +0 and -0),
# near-axis suns, a sun below the horizon
SUNS = {f"oct{''.join('+' if s > 0 else '-' for s in o)}": (0.35 * o[0], 0.8 * o[1], 0.45 * o[2])
        for o in [(x, y, z) for x in (1, -1) for y in (1, -1) for z in (1, -1)]}
SUNS.update({"zero_x": (0.0, 0.8, 0.6), "negzero_z": (0.6, 0.8, -0.0), "zero_xz": (0.0, 1.0, 0.0),
             "near_axis": (1e-9, 1.0, -1e-9), "below": (0.3, -0.9, 0.3)})

SHAPES = ((64, 48), (33, 33))


def params(sun=None, textured=False, **kw):
    if sun is not None:
        kw["sun_dir"] = sun
    p = vrt.default_params(4, 4, **kw)
    return vrt.textured_params(p, ref_atlas(), 128) if textured else p


def run_cases(name, n, cases, trees=(0,), textured=False, with_oracle=False):
    """cases: (id, camera keywords, sun or None). Each as a plain launch per trees mode; consecutive
    cases pairwise as a frame batch of two different cameras (the sun is a launch's: the pair takes the
    first case's)."""
    vox = volumes(n)[name]
    near = 0
    with vrt.Renderer(0) as r:
        r.upload_volume(vox, n)
        for w, h in SHAPES:
            cams = [vrt.make_camera(w, h, **kw) for _, kw, _ in cases]
            for i, (cid, _, sun) in enumerate(cases):
                p = params(sun, textured)
                reset_modes(r)
                ref = band(r, cams[i], p, counters=True)
                j = (i + 1) % len(cases)
                p2 = [params(sun, textured, time=1.0), params(sun, textured, time=2.0)]
                ref2 = [band(r, cams[i], p2[0], counters=True), band(r, cams[j], p2[1], counters=True)]
                for t in trees:
                    certified_mode(r, t)
                    assert_equal(band(r, cams[i], p), ref, (name, n, cid, (w, h), "plain", t))
                    if not textured:  # frame batches are colour-only launches
                        got2 = batch(r, [cams[i], cams[j]], p2)
                        for f in range(2):
                            assert_equal(got2[f], ref2[f], (name, n, cid, (w, h), "batch", t, f))
                if with_oracle and n == 16 and (w, h) == SHAPES[0]:
                    rgba_o, _, _ = oracle.render(cams[i], vox, n, p, threads=THREADS)
                    near += check_raw(words_to_bytes(ref), rgba_o)
    return near


@pytest.mark.parametrize("n", (16, 32))
@pytest.mark.parametrize("name", ("shell", "glass_clutter"))
def test_start_cases(built, name, n):
    cases = [(cid, kw, None) for cid, kw in start_cameras(n).items()]
    near = run_cases(name, n, cases, with_oracle=True)
    print(f"{name} {n}: {near} bytes one LSB from the oracle's")


@pytest.mark.parametrize("n", (16, 32))
@pytest.mark.parametrize("name", ("shell", "glass_clutter"))
def test_sun_cases(built, name, n):
    """Every face orientation lit and shaded: a camera inside the shell, one outside the clutter."""
    cam = start_cameras(n)
    views = (cam["lattice_half_diag"], cam["lattice_down"], cam["outside_pz"])
    cases = [(sid, views[i % len(views)], sun) for i, (sid, sun) in enumerate(SUNS.items())]
    run_cases(name, n, cases)


def test_trees_on_glass_clutter(built):
    n = 16
    cam = start_cameras(n)
    cases = [("lattice_axis", cam["lattice_axis"], SUNS["oct+++"]), ("outside_px", cam["outside_px"], SUNS["oct-+-"]),
             ("lattice_down", cam["lattice_down"], SUNS["zero_x"]), ("straight_down", cam["straight_down"], SUNS["below"])]
    run_cases("glass_clutter", n, cases, trees=(2,))


@pytest.mark.parametrize("name,n", (("shell", 16), ("glass_clutter", 32)))
def test_textured_reference_atlas(built, name, n):
    cam = start_cameras(n)
    cases = [("lattice_half_diag", cam["lattice_half_diag"], SUNS["oct+++"]), ("outside_nz", cam["outside_nz"], SUNS["oct--+"]),
             ("lattice_axis_int", cam["lattice_axis_int"], SUNS["negzero_z"]), ("outside_py", cam["outside_py"], SUNS["oct-++"])]
    run_cases(name, n, cases, textured=True)
