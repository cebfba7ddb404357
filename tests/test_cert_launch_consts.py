"""The certified pass's launch constants (KArgs::setup and the fields behind its flags, KArgs::fw .. max_len2;
cert_launch_consts and setup_consts in csrc/vrt_launch_consts.cpp, through the library's host-only test hook)
against a NumPy float32 restatement of primary_ray's vertex stage and start (csrc/vrt_render.hip) over
every pixel of small frames and the corner and centre pixels of large ones.

Where the host sets a flag, the kernel drops per-pixel work on the strength of a proof; here the proved
property is asserted pixel by pixel on the kernel's own floats:
 - kSetupW: n4.w and f4.w are the launch's wn and wf bit for bit, the reciprocals are 1 / w;
 - kSetupLen: the squared length of vdir takes normalize3's rcp_newton(sqrt_fix(s)) with no range test;
 - kSetupCell: floor(P) is the launch's cell (inside the volume), the three plane tests of cert_pixel's
   start hold for either direction sign, no on-plane trigger fires, and the supplied fl + 1 is
   floor(+-P) + 1.
Cameras that must set every flag, cameras that must clear the flag concerned, and the wave-uniform float
work of setup_consts against the kernel's expressions."""
import numpy as np
import pytest

import voxelraytracer_amd as vrt
from harness import ALL, K_CELL, K_LEN, K_W, consts, float_bits as bits

F = np.float32
RNG = np.random.default_rng(20311)
SMALL = ((64, 48), (96, 54))
LARGE = ((1920, 1080), (32768, 8))


def matrix(w, h, **kw):
    return np.array(vrt.make_camera(w, h, **kw).inv_pv, np.float32)


def pixels_of(w, h):
    if w * h <= 96 * 54:
        py, px = np.mgrid[0:h, 0:w]
        return px.reshape(-1), py.reshape(-1)
    px = np.array([0, w - 1, 0, w - 1, w // 2])
    py = np.array([0, 0, h - 1, h - 1, h // 2])
    return px, py


def vertex_stage(m, n, w, h, px, py):
    """primary_ray's floats for the pixels (px, py): n4.w, f4.w, the squared length of vdir and P."""
    m = np.asarray(m, np.float32)
    with np.errstate(all="ignore"):
        ndx = (F(2) * (px.astype(np.float32) + F(0.5))) / F(w) - F(1)
        ndy = (F(2) * (py.astype(np.float32) + F(0.5))) / F(h) - F(1)
        n4, f4 = [], []
        for i in range(4):
            base = m[i] * ndx + m[4 + i] * ndy
            n4.append((base + m[8 + i] * F(-1)) + m[12 + i] * F(1))
            f4.append((base + m[8 + i] * F(1)) + m[12 + i] * F(1))
        vnear = [n4[i] / n4[3] for i in range(3)]
        vdir = [f4[i] / f4[3] - vnear[i] for i in range(3)]
        half = F(n) * F(0.5)
        P = np.stack([v + half for v in vnear], axis=1)
        s = (vdir[0] * vdir[0] + vdir[1] * vdir[1]) + vdir[2] * vdir[2]
    return n4[3], f4[3], s, P


def expo(x):
    return (bits(x) >> 23) & 0xFF


def check_pixels(m, n, w, h, k):
    """Every property a set flag stands for, on every pixel of the frame (or its corners and centre)."""
    px, py = pixels_of(w, h)
    nw, fw_, s, P = vertex_stage(m, n, w, h, px, py)
    if k["setup"] & K_W:
        assert k["vdiv_ok"] == 1
        assert (bits(nw) == bits(k["wn"])).all() and (bits(fw_) == bits(k["wf"])).all()
        assert bits(k["rcp_wn"]) == bits(F(1) / k["wn"]) and bits(k["rcp_wf"]) == bits(F(1) / k["wf"])
        for v in (k["wn"], k["wf"]):  # markstein_safe(d)
            assert 2.0 ** -60 <= abs(float(v)) <= 2.0 ** 60
    else:
        assert not k["setup"] & (K_LEN | K_CELL)  # both build on the constant w
    if k["setup"] & K_LEN:
        b = bits(s).astype(np.int64)
        assert not (np.abs(b - 0x3F800000) <= 1024).any()             # outside normalize3's near-one window
        assert ((expo(s) >= 95) & (expo(s) <= 252)).all()             # sqrt_fix_ok(s)
        root = np.sqrt(s)
        assert ((expo(root) >= 2) & (expo(root) <= 252)).all()        # rcp_rn_ok(sqrt(s))
    if k["setup"] & K_CELL:
        c = k["cell"]
        assert ((c >= 0) & (c < n)).all()
        assert (np.floor(P) == c.astype(np.float32)).all()
        for q, fl1 in ((P, k["fl1_up"]), (-P, k["fl1_dn"])):          # moving up, moving down
            fl = np.floor(q)
            assert (fl + F(1) == fl1).all()                            # the supplied floor + 1
            assert (np.floor(q + F(1)) == fl + F(1)).all()             # the plane tests
            assert (fl != q).all()                                     # no on-plane trigger
        assert (k["fl1_up"] == (c + 1).astype(np.float32)).all() and (k["fl1_dn"] == (-c).astype(np.float32)).all()
        # the margin of the proof: every P is at least 2^-10 cell from a plane
        assert (np.minimum(P - np.floor(P), np.ceil(P) - P) >= 2.0 ** -10).all()


def run(n, kw=None, edit=None, shapes=SMALL + LARGE):
    """The flags per frame shape for a camera (keywords of make_camera; edit: a function of the matrix),
    with the per-pixel assertions wherever a flag is set."""
    flags = {}
    for w, h in shapes:
        m = matrix(w, h, **(kw or {}))
        if edit is not None:
            m = edit(m.copy())
        k = consts(m, n, w, h)
        check_pixels(m, n, w, h, k)
        flags[(w, h)] = k["setup"]
    return flags


# ---- cameras that must set every flag ---------------------------------------------------------

@pytest.mark.parametrize("n", (16, 32, 128))
def test_default_camera_sets_every_flag(n):
    flags = run(n)
    for shape in SMALL + ((1920, 1080),):
        assert flags[shape] == ALL, (n, shape, flags[shape])
    # 32768x8: the near points of a 4096:1 frame span many cells; w and the length range still hold
    assert flags[(32768, 8)] == K_W | K_LEN


def test_default_camera_constants_at_128():
    """The figures the change was planned on: w = 100 and 0.00999832, the start cell (60, 66, 67)."""
    k = consts(matrix(1920, 1080), 128, 1920, 1080)
    assert k["setup"] == ALL
    assert k["wn"] == F(100.0) and abs(float(k["wf"]) - 0.00999832) < 1e-8
    assert k["cell"].tolist() == [60, 66, 67]


def random_poses(n, count):
    """Poses inside the volume whose position is at least 0.1 cell from every cell plane (the near points of
    a 90 degree 16:9 frame spread 0.018 cell around the position's near point, 0.01 ahead of it)."""
    for _ in range(count):
        cell = RNG.integers(-n // 2 + 1, n // 2 - 1, 3)
        pos = cell + RNG.uniform(0.1, 0.9, 3)
        rot = (RNG.uniform(-85, 85), RNG.uniform(-180, 180), RNG.uniform(-30, 30))
        yield dict(pos=tuple(float(x) for x in pos), rot=tuple(float(x) for x in rot))


def test_random_poses_inside_the_volume_set_every_flag():
    cells = set()
    for i, kw in enumerate(random_poses(32, 64)):
        flags = run(32, kw, shapes=SMALL + ((1920, 1080),))
        assert all(f == ALL for f in flags.values()), (kw, flags)
        cells.add(tuple(consts(matrix(64, 48, **kw), 32, 64, 48)["cell"].tolist()))
    assert len(cells) > 40


# ---- cameras that must clear the flag concerned ------------------------------------------------

def start_x(kw, n, w=64, h=48):
    px, py = pixels_of(w, h)
    return vertex_stage(matrix(w, h, **kw), n, w, h, px, py)[3][:, 0]


def test_start_on_or_near_a_plane_clears_the_cell_flag():
    n = 32
    # yaw 90: the near plane is an x plane, every pixel's P.x is the same up to rounding (asserted), 0.01 from pos.x + 16
    view = dict(rot=(0.0, 90.0, 0.0))
    x0 = start_x(dict(pos=(3.3, 0.4, 0.6), **view), n)
    assert x0.max() - x0.min() < 1e-5
    off = float(x0.mean()) - 3.3
    cases = {
        "exactly_on": 19.0 - off,            # P.x = 19 for some pixels (asserted below)
        "within_1e-3_above": 19.0005 - off,
        "within_1e-3_below": 18.9995 - off,
    }
    for name, x in cases.items():
        kw = dict(pos=(x, 0.4, 0.6), **view)
        px_ = start_x(kw, n)
        assert np.abs(px_ - 19.0).min() < 1e-3, name
        for shape, f in run(n, kw).items():
            assert f & K_W and not f & K_CELL, (name, shape, f)
    found = False  # some float position puts a pixel's P.x exactly on the plane
    for x in np.nextafter(F(cases["exactly_on"]), F(100.0)) + np.arange(-64, 64) * np.spacing(F(3.0)):
        if (start_x(dict(pos=(float(x), 0.4, 0.6), **view), n) == F(19.0)).any():
            found = True
            assert not run(n, dict(pos=(float(x), 0.4, 0.6), **view), shapes=SMALL)[(64, 48)] & K_CELL
            break
    assert found
    # 2e-2 from the plane the same camera sets the flag: the cases above are cleared by the plane alone
    assert run(n, dict(pos=(19.3 - off, 0.4, 0.6), **view), shapes=SMALL)[(64, 48)] == ALL


def test_near_point_spread_across_a_plane_clears_the_cell_flag():
    n = 32
    kw = dict(pos=(2.004, 0.37, -1.45), rot=(-20.0, 0.0, 0.0))  # yaw 0: P.x spreads +-0.013 around 18.004
    x = start_x(kw, n)
    assert len(np.unique(np.floor(x))) == 2
    for shape, f in run(n, kw).items():
        assert f & K_W and f & K_LEN and not f & K_CELL, (shape, f)


@pytest.mark.parametrize("axis,sign", [(a, s) for a in range(3) for s in (1, -1)])
def test_camera_outside_the_volume_clears_the_cell_flag(axis, sign):
    n = 16
    pos = [0.3, 0.4, 0.6]
    pos[axis] = sign * (n / 2 + 3.5)
    for shape, f in run(n, dict(pos=tuple(pos))).items():
        assert f & K_W and f & K_LEN and not f & K_CELL, (shape, f)


def set_entry(i, v):
    def edit(m):
        m[i] = v
        return m
    return edit


def test_w_threshold():
    """m11 is about -50 for the default projection: ulp / 4 = 9.5e-7. Below it the flag holds, above it
    the flag clears; the per-pixel assertions hold in either state (run)."""
    m = matrix(64, 48)
    assert 32.0 <= abs(float(m[11])) < 64.0
    for n in (16, 128):
        below = run(n, edit=set_entry(3, 1e-8))
        above = run(n, edit=set_entry(3, 1e-6))
        coarse = run(n, edit=set_entry(3, 1e-3))
        for shape in SMALL + LARGE:
            assert below[shape] & K_W, shape
            assert above[shape] == 0 and coarse[shape] == 0, shape
        assert run(n, edit=set_entry(7, -1e-6))[(64, 48)] == 0
    # with the x term large enough to reach n4.w, the pixels do differ: the flag is needed
    px, py = pixels_of(64, 48)
    m[3] = 1e-3
    nw = vertex_stage(m, 16, 64, 48, px, py)[0]
    assert len(np.unique(bits(nw))) > 1


def test_non_finite_entries_clear_every_flag():
    for i in range(16):
        for v in (np.nan, np.inf, -np.inf):
            for shape, f in run(32, edit=set_entry(i, v), shapes=SMALL).items():
                assert f == 0, (i, v, shape)
    k = consts(np.zeros(16, np.float32), 32, 64, 48)
    assert k["setup"] == 0


def scale_xyz(f):
    def edit(m):
        for i in (0, 1, 2):
            m[i::4] *= F(f)
        return m
    return edit


def test_scaled_matrix_leaves_the_length_range():
    n = 32
    px, py = pixels_of(64, 48)
    for f, outside in ((1e-3, lambda s: s < 4.0), (2.0 ** 48, lambda s: s > 2.0 ** 98)):
        m = scale_xyz(f)(matrix(64, 48))
        assert outside(vertex_stage(m, n, 64, 48, px, py)[2].astype(np.float64)).all()
        # (not the 4096:1 frame: its x column times 2^48 leaves the vertex divisions' own range)
        for shape, fl in run(n, edit=scale_xyz(f), shapes=SMALL + ((1920, 1080),)).items():
            assert fl & K_W and not fl & K_LEN, (f, shape, fl)
    # a squared length inside normalize3's near-one window, where the closed form must run
    m = scale_xyz(1.0 / 100.0)(matrix(64, 48))
    assert not consts(m, n, 64, 48)["setup"] & K_LEN
    # beyond the vertex divisions' own range nothing is set
    assert run(n, edit=scale_xyz(2.0 ** 60), shapes=SMALL)[(64, 48)] == 0


def test_frame_batches_need_one_matrix():
    m = matrix(64, 48)
    m2 = matrix(64, 48, pos=(1.3, 0.4, 0.6))
    assert consts(m, 32, 64, 48, m2=m.copy())["setup"] == ALL
    assert consts(m, 32, 64, 48, m2=m2)["setup"] == 0
    assert consts(m2, 32, 64, 48, m2=m)["setup"] == 0
    bad = m.copy()
    bad[5] = np.nan
    assert consts(m, 32, 64, 48, m2=bad)["setup"] == 0


# ---- the wave-uniform float work ---------------------------------------------------------------

def test_setup_consts_are_the_kernels_expressions():
    k24 = F(2.0) * F(2.0 ** -24)
    m = matrix(64, 48)
    for n in (2, 16, 128, 1024):
        for w, h in SMALL + LARGE + ((33, 33), (1, 1)):
            for max_len in (100.0, 0.0, 1e-3, 16777216.0, 3e38, float("inf")):
                k = consts(m, n, w, h, max_len=max_len)
                fn = F(n)
                with np.errstate(over="ignore"):
                    want = np.array([F(w), F(h), fn * F(0.5), k24 * (F(3.0) * fn + F(11.0)), F(max_len) + F(2.0)], np.float32)
                got = np.array([k["fw"], k["fh"], k["half_n"], k["walk_b0"], k["max_len2"]], np.float32)
                assert np.array_equal(bits(got), bits(want)), (n, w, h, max_len, got, want)
