"""CPU restatements, in NumPy float32, of the forms the certified pass takes once per pixel around its
two walks (csrc/vrt_cert.h) beside the forms they replace:
 - cert_pixel's start: exact_start_cell's floor / ceil - 1 cell with its plane tests against the
   sign-folded cell int(floor(s P)) ^ m with the plane test floor(q + 1) == floor(q) + 1, and
   start_layers_clear's per-axis entry condition against the on-plane trigger;
 - cert_shade_hit's lit term: dot3 / reflect3 / dot3 on the face normal against the axis form;
 - the sun's launch constants (KArgs::sun_*, sun_consts in vrt_launch_consts.cpp, through the library's test
   hook) against the kernel's expressions.
float -> int is v_cvt_i32_f32: NaN gives 0, values beyond the range saturate."""
import ctypes as C
import itertools

import numpy as np

RNG = np.random.default_rng(20261)
F = np.float32


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cvt_i32(x):
    """v_cvt_i32_f32 of an integral (or special) float32, as int64 holding the int32 value."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        y = np.where(np.isnan(x), F(0), x).astype(np.float64)
    return np.clip(y, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def wrap32(i):
    return ((np.asarray(i, np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def fast_ok(d):
    with np.errstate(invalid="ignore"):
        a = np.abs(d)
        return (a >= F(2.0 ** -64)) & (a <= F(1.0e4))


def positions(n):
    """Integers, half-integers and +-1, 2 ulp around the integers near the volume's faces and inside it,
    and the special values."""
    ints = np.array([-2, -1, 0, 1, 2, 3, 7, 8, n // 2, n - 2, n - 1, n, n + 1, n + 2], np.float32)
    base = np.concatenate([ints, ints + F(0.5), -ints, np.array([0.25, 1e-30, -1e-30, 2.0 ** 24, -(2.0 ** 24)], np.float32)])
    b = bits(base).astype(np.int64)
    near = np.concatenate([b + k for k in (-2, -1, 0, 1, 2)]) & 0xFFFFFFFF
    special = f32(np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x00000001,
                            0x80000001], np.uint32))
    big = np.array([2.0 ** 31, -(2.0 ** 31), 2.0 ** 31 + 256, -(2.0 ** 31) - 256, 2.0 ** 32, 3e38, -3e38], np.float32)
    return np.unique(np.concatenate([f32(near.astype(np.uint32)), special, big]).view(np.uint32)).view(np.float32)


DIRS = np.concatenate([
    np.array([0.0, 2.0 ** -65, 2.0 ** -64, 1e-12, 0.3, 0.57735, 1.0, 1.0e4, 1.0001e4, np.inf], np.float32),
    -np.array([0.0, 2.0 ** -65, 2.0 ** -64, 1e-12, 0.3, 0.57735, 1.0, 1.0e4, 1.0001e4, np.inf], np.float32),
    f32(np.array([0x7FC00000], np.uint32)),
])


def old_axis(p, d, n):
    """exact_start_cell on one axis: (cell, bounds and plane hold), and start_layers_clear's entry."""
    with np.errstate(invalid="ignore", over="ignore"):
        up = d > 0
        c = wrap32(np.where(up, cvt_i32(np.floor(p)), cvt_i32(np.ceil(p)) - 1))
        wp = np.where(up, np.floor(p + F(1)), np.ceil(p - F(1)))
        inb = (c & 0xFFFFFFFF) < n
        plane = wp == wrap32(c + up.astype(np.int64)).astype(np.float32)
        entry = (d < 0) & (p == np.floor(p))
    return c, inb & plane, entry


def new_axis(p, d, n):
    """cert_pixel<LEAN>'s sign-folded start on one axis."""
    with np.errstate(invalid="ignore", over="ignore"):
        up = d > 0
        q = np.where(up, p, -p)
        f = np.floor(q)
        m = np.where(up, 0, -1).astype(np.int64)
        c = wrap32(cvt_i32(f) ^ m)
        inb = (c & 0xFFFFFFFF) < n
        plane = np.floor(q + F(1)) == f + F(1)
        entry = ~up & (f == q)
    return c, inb & plane, entry


def test_start_cell_one_axis_grid():
    """Every position against every direction component, per axis: the same verdict, the same cell
    whenever the verdict holds, and the same entry condition wherever the component is in the
    fast-path range (elsewhere the merged predicate is false and the trigger is not looked at)."""
    for n in (16, 128, 1024):
        P = positions(n)
        p, d = [a.reshape(-1) for a in np.meshgrid(P, DIRS, indexing="ij")]
        co, oo, eo = old_axis(p, d, n)
        cn, on, en = new_axis(p, d, n)
        ok_d = fast_ok(d)
        assert np.array_equal(oo & ok_d, on & ok_d)
        assert np.array_equal(co[oo & ok_d], cn[on & ok_d])
        assert np.array_equal(eo[ok_d], en[ok_d])
        # and where a zero or NaN component makes `d < 0` and `!(d > 0)` differ, nowhere else
        assert not ok_d[eo != en].any()
        assert (oo & ok_d).any() and (~oo & ok_d).any() and (eo & oo & ok_d).any()
        # cells -1 and N appear among the rejected starts (a camera outside the volume)
        rej = ok_d & ~on
        assert (cn[rej] == -1).any() and (cn[rej] == n).any()


def test_start_predicate_triples():
    """The whole predicate on triples: fast_path_ok(D), bounds and planes of three axes ANDed, and the
    trigger: start_layers_clear is entered exactly when the old code entered its per-axis block."""
    n = 128
    P = positions(n)
    octants = np.array(list(itertools.product(DIRS, repeat=3)), np.float32)  # every sign pattern, +-0 included
    k = len(octants) * 40
    D = np.tile(octants, (40, 1))
    Pt = P[RNG.integers(0, len(P), (k, 3))]
    inside = RNG.integers(0, 2, (k, 3)).astype(bool)      # half of the coordinates inside the volume, on or near planes
    cand = P[(P >= 0) & (P < n)]
    Pt = np.where(inside, cand[RNG.integers(0, len(cand), (k, 3))], Pt)
    old = [old_axis(Pt[:, a], D[:, a], n) for a in range(3)]
    new = [new_axis(Pt[:, a], D[:, a], n) for a in range(3)]
    fok = fast_ok(D[:, 0]) & fast_ok(D[:, 1]) & fast_ok(D[:, 2])
    ok_old = fok & old[0][1] & old[1][1] & old[2][1]
    ok_new = fok & new[0][1] & new[1][1] & new[2][1]
    assert np.array_equal(ok_old, ok_new)
    for a in range(3):
        assert np.array_equal(old[a][0][ok_old], new[a][0][ok_new])
    trig_old = ok_old & (old[0][2] | old[1][2] | old[2][2])
    trig_new = ok_new & (new[0][2] | new[1][2] | new[2][2])
    assert np.array_equal(trig_old, trig_new)
    assert ok_old.sum() > 1000 and trig_old.sum() > 100 and (ok_old & ~trig_old).sum() > 100


def test_first_planes_from_the_start_floats():
    """The walk's first planes from the start's floored floats, ((fl + 1) - Ps) |rcp|, are (float(c + u) -
    P) rcp bit for bit for every start the predicate accepts, and never negative: no plane behind the start."""
    n = 1024
    k = 1_000_000
    P = np.concatenate([RNG.uniform(0, n, k).astype(np.float32), positions(n)])
    P = P[(P >= 0) & (P < n)]
    rm = f32(RNG.integers(0x2F800000, 0x5F800000, len(P), dtype=np.uint64).astype(np.uint32))
    for up in (True, False):
        d = np.where(up, F(0.5), F(-0.5)) * np.ones(len(P), np.float32)
        c, ok, _ = old_axis(P, d, n)
        rcp = rm if up else -rm
        old = ((c + (1 if up else 0)).astype(np.float32) - P) * rcp
        q = P if up else -P
        new = ((np.floor(q) + F(1)) - q) * np.abs(rcp)
        assert np.array_equal(bits(old[ok]), bits(new[ok]))
        assert (new >= 0).all() and not np.signbit(new[ok]).any()


def lit_generic(S, D, a):
    """lit_brightness's two dot products on hh.normal = -sign(D_a) e_a (cert_hit_record)."""
    with np.errstate(under="ignore"):
        nrm = np.zeros_like(D)
        nrm[np.arange(len(D)), a] = -np.sign(D[np.arange(len(D)), a])
        dot = lambda u, v: (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]
        ns = dot(nrm, S)
        s = F(2) * ns
        R = S - s[:, None] * nrm
        return ns, dot(R, D)


def lit_axis(S, D, a):
    with np.errstate(under="ignore"):
        i = np.arange(len(D))
        ns = np.where(D[i, a] > 0, -S[i, a], S[i, a])
        p = S * D
        p[i, a] = -p[i, a]
        return ns, (p[:, 0] + p[:, 1]) + p[:, 2]


def unit_dirs(k):
    v = RNG.normal(size=(k, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v = v.astype(np.float32)
    return v[(np.abs(v) >= 2.0 ** -64).all(axis=1)]


def suns_nonzero():
    mags = np.array([2.0 ** -64, 2.0 ** -63, 1e-12, 1e-4, 0.1, 0.301511, 0.57735, 0.904534, 1.0], np.float32)
    tri = np.array(list(itertools.product(mags, repeat=3)), np.float32)
    signs = np.array(list(itertools.product([1, -1], repeat=3)), np.float32)
    return (tri[:, None, :] * signs[None, :, :]).reshape(-1, 3)


def test_lit_term_axis_form_is_bitwise_the_generic_form():
    """All six faces (three axes, both signs of D_a among the random directions), suns in all eight
    octants with components from 1 down to 2^-64, a few thousand unit directions."""
    S0 = suns_nonzero()
    D0 = unit_dirs(3000)
    assert len(D0) > 2900
    for a in range(3):
        si = RNG.integers(0, len(S0), 400_000)
        di = RNG.integers(0, len(D0), 400_000)
        S, D = S0[si], D0[di]
        av = np.full(len(S), a)
        assert (D[:, a] > 0).any() and (D[:, a] < 0).any()
        g_ns, g_sp = lit_generic(S, D, av)
        x_ns, x_sp = lit_axis(S, D, av)
        assert np.array_equal(bits(g_ns), bits(x_ns))
        assert np.array_equal(bits(g_sp), bits(x_sp))
    # every sun against a fixed set of directions, every octant of both
    D = np.array(list(itertools.product([0.57735, -0.57735], repeat=3)), np.float32)
    for a in range(3):
        S, Dd = np.repeat(S0, len(D), axis=0), np.tile(D, (len(S0), 1))
        av = np.full(len(S), a)
        g, x = lit_generic(S, Dd, av), lit_axis(S, Dd, av)
        assert np.array_equal(bits(g[0]), bits(x[0])) and np.array_equal(bits(g[1]), bits(x[1]))


def test_a_zero_in_the_sun_needs_the_guard():
    """A search over suns with a zero component (both signs of zero) finds forms that differ, in the sign
    of a zero: the wave-uniform guard (KArgs::sun_ok) is needed; nothing else differs there."""
    vals = np.array([0.0, -0.0, 0.6, -0.6, 0.8, -0.8, 1.0, -1.0], np.float32)
    S0 = np.array([s for s in itertools.product(vals, repeat=3) if 0.0 in np.abs(s) and np.any(np.abs(s) > 0)], np.float32)
    D = np.array(list(itertools.product([0.57735, -0.57735], repeat=3)), np.float32)
    found = 0
    for a in range(3):
        S, Dd = np.repeat(S0, len(D), axis=0), np.tile(D, (len(S0), 1))
        av = np.full(len(S), a)
        g, x = lit_generic(S, Dd, av), lit_axis(S, Dd, av)
        for u, v in zip(g, x):
            diff = bits(u) != bits(v)
            found += int(diff.sum())
            assert np.array_equal(u, v)                       # equal in value everywhere
            assert ((u[diff] == 0) & (v[diff] == 0)).all()   # bits differ only where both are zeros
    assert found > 0


def test_sun_constants_from_the_host():
    """KArgs::sun_* as make_args fills them (vrt_debug_sun_consts, host arithmetic) against the kernel's
    expressions on normalize(sun_dir): fast_path_ok, cert_walk's step signs, sign fold, octant and
    |S|_1 with its products by k24 = 2 * 2^-24, in the kernel's order."""
    import voxelraytracer_amd as vrt

    lib = vrt.lib()
    fn = lib.vrt_debug_sun_consts
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    suns = [np.array(s, np.float32) * np.array(o, np.float32)
            for s in ((0.3, 0.9, 0.3), (1.0, 2.0, 3.0), (1e-3, 5.0, 1e-3), (1.0, 1e-25, 1.0), (0.5, 0.5, 0.5))
            for o in itertools.product([1, -1], repeat=3)]
    suns += [np.array(s, np.float32) for s in ((0.0, 1.0, 0.5), (0.3, -0.0, 0.3), (0.0, -1.0, 0.0), (1.0, 0.0, -0.0),
                                                (0.3, -0.9, 0.3), (1e30, 1.0, 1.0))]
    suns += [RNG.normal(size=3).astype(np.float32) for _ in range(200)]
    ostride = 2 * 129 ** 3
    some_not_ok = 0
    for s in suns:
        out = np.zeros(12, np.uint32)
        assert fn(s.ctypes.data, ostride, out.ctypes.data) == 0
        with np.errstate(divide="ignore", over="ignore", invalid="ignore", under="ignore"):
            inv = F(1) / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
            sn = s * inv
            ok = bool(fast_ok(sn).all())
            neg = np.where(sn > 0, 0, 0x80000000).astype(np.uint32)
            step = np.where(sn > 0, 1, -1).astype(np.int32)
            obase = np.uint32((int(sn[0] < 0) | int(sn[1] < 0) << 1 | int(sn[2] < 0) << 2) * ostride)
            k24 = F(2.0) * F(2.0 ** -24)
            l1 = (np.abs(sn[0]) + np.abs(sn[1])) + np.abs(sn[2])
            q2 = (F(0.5) * k24) * l1
            b1 = k24 * l1
            g2 = F(2.0) * q2
        some_not_ok += not ok
        assert out[0] == int(ok), s
        assert np.array_equal(out[1:4], neg), s
        assert np.array_equal(out[4:7].view(np.int32), step), s
        assert out[7] == obase, s
        want = np.array([l1, q2, b1, g2], np.float32)
        assert np.array_equal(out[8:12], bits(want)), (s, out[8:12].view(np.float32), want)
        if ok:  # the sign fold by xor is the kernel's select ux ? P : -P
            P = np.array([3.25, -0.0, 17.0], np.float32)
            assert np.array_equal(bits(P) ^ neg, bits(np.where(sn > 0, P, -P)))
    assert some_not_ok >= 4
