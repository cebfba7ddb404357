"""CPU restatements, in NumPy float32, of the forms the certified pass takes on the shadow side of a primary
hit (csrc/vrt_cert.h: cert_hit_record_primary, cert_shade_hit<.., KAX>, cert_start_sun and the prologue of
cert_walk<true, LEAN, true, KSUN>) beside the forms they replace. Every pair must agree bit for bit:
 - cert_start_sun against cert_start: the predicate, ed, and the first planes it keeps for the walk against
   the planes the walk's prologue formed itself (u_b from the sun's sign there, from KArgs::sun_step here);
 - the predicate's integer | and & against || and &&, over the whole truth table;
 - the record's len = u against 0 + u, and the colour y against mixf(+0, y, 1);
 - start_texel's value against path_texel's;
 - the air cell's "moved off the start cell" test by xor / or against the comparison of the cells.
Inputs: the eight sun octants (both step signs per axis), both signs of the ray on every axis, each face
axis, hit points on and one and two ulps beside integer planes, zero and -0 components."""
import ctypes as C
import itertools

import numpy as np

RNG = np.random.default_rng(20262)
F = np.float32


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def f32(b):
    return np.asarray(b, np.uint32).view(np.float32)


def sun_consts(sun):
    """KArgs::sun_ok, sun_neg[3], sun_step[3] and normalize(sun) with its reciprocals, as the host fills them."""
    import voxelraytracer_amd as vrt

    fn = vrt.lib().vrt_debug_sun_consts
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
    s = np.array(sun, np.float32)
    out = np.zeros(12, np.uint32)
    assert fn(s.ctypes.data, 2 * 129 ** 3, out.ctypes.data) == 0
    with np.errstate(all="ignore"):
        sn = s * (F(1) / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]))
        rcp = F(1) / sn
    return int(out[0]), out[1:4].copy(), out[4:7].view(np.int32).copy(), sn.astype(np.float32), rcp.astype(np.float32)


OCTANTS = list(itertools.product([1.0, -1.0], repeat=3))
SUNS = [(0.35 * o[0], 0.8 * o[1], 0.45 * o[2]) for o in OCTANTS] + [(1e-3 * o[0], 1.0 * o[1], 2e-3 * o[2]) for o in OCTANTS]


def hit_points(n):
    """Coordinates on integer planes of the volume, one and two ulps beside them, on half-integers, inside
    cells, and the two zeros."""
    ints = np.array([0, 1, 2, 7, n // 2, n - 1, n], np.float32)
    b = bits(np.concatenate([ints, ints + F(0.5), ints + F(0.25), ints + F(0.999)])).astype(np.int64)
    near = np.concatenate([b + k for k in (-2, -1, 0, 1, 2)])
    near = near[near >= 0]
    return np.unique(np.concatenate([f32(near.astype(np.uint32)), f32(np.array([0x00000000, 0x80000000], np.uint32))]).view(np.uint32)).view(np.float32)


def cases(n, k):
    """k random combinations: hit point X (each coordinate from hit_points), the start cell beside it (floor
    of X and its two neighbours per axis), the ray D0 (all sign octants, magnitudes down to 2^-10), the face
    axis and the primary walk's bound e."""
    P = hit_points(n)
    X = P[RNG.integers(0, len(P), (k, 3))]
    cell = np.floor(X).astype(np.int64) + RNG.integers(-1, 2, (k, 3))
    mag = np.array([2.0 ** -10, 1e-2, 0.3, 0.57735, 0.8, 1.0], np.float32)
    D0 = mag[RNG.integers(0, len(mag), (k, 3))] * np.array(OCTANTS, np.float32)[RNG.integers(0, 8, k)]
    fa = RNG.integers(0, 3, k)
    e = np.array([0.0, 1e-7, 1e-6, 1e-4, 4e-3], np.float32)[RNG.integers(0, 5, k)]
    return X, cell, D0.astype(np.float32), fa, e


def cert_start_old(X, D0, Dn, rcpn, fa, e, cell):
    """cert_start: (verdict, ed)."""
    i = np.arange(len(X))
    with np.errstate(all="ignore"):
        ed = F(2) * e[:, None] * np.abs(D0 * rcpn)
        d0a, rna = D0[i, fa], np.broadcast_to(rcpn, X.shape)[i, fa]
        lead = (e * np.abs(d0a) + F(1e-5)) * np.abs(rna)
        w = ((cell + (Dn > 0)).astype(np.float32) - X) * rcpn
        fr = X - np.floor(X)
        dm = e[:, None] * np.abs(D0) + F(2e-5)
        ok = np.ones(len(X), bool)
        for b in range(3):
            okb = (fa == b) | ((w[:, b] >= lead + ed[:, b] + F(1e-4)) & (fr[:, b] >= dm[:, b]) & (F(1) - fr[:, b] >= dm[:, b]))
            ok &= okb
    return ok, ed


def walk_planes_old(X, rcp, cell, step):
    """The prologue of cert_walk with the sun's constants: sig_b = (float(c_b + u_b) - P_b) rcp_b, u_b = step_b > 0."""
    with np.errstate(all="ignore"):
        return ((cell + (step > 0)).astype(np.float32) - X) * rcp


def cert_start_sun(X, D0, d0a, step, rcpn, fa, e, cell):
    """cert_start_sun: (verdict, ed, the planes it hands the walk)."""
    with np.errstate(all="ignore"):
        ed = F(2) * e[:, None] * np.abs(D0 * rcpn)
        rna = np.broadcast_to(rcpn, X.shape)[np.arange(len(X)), fa]
        lead = (e * np.abs(d0a) + F(1e-5)) * np.abs(rna)
        u = np.where(step > 0, 1, 0)
        sig = ((cell + u).astype(np.float32) - X) * rcpn
        fr = X - np.floor(X)
        dm = e[:, None] * np.abs(D0) + F(2e-5)
        okb = [(fa == b).astype(np.int32) | ((sig[:, b] >= lead + ed[:, b] + F(1e-4)).astype(np.int32) &
                                             (fr[:, b] >= dm[:, b]).astype(np.int32) &
                                             (F(1) - fr[:, b] >= dm[:, b]).astype(np.int32)) for b in range(3)]
    return (okb[0] & okb[1] & okb[2]) != 0, ed, sig


def test_shadow_start_against_cert_start_and_the_walks_planes():
    """Every sun octant (two magnitude patterns each) against 60 000 hits: the same verdict, the same ed, and
    planes that are both cert_start's w_b and the walk's own sig_b, bit for bit; verdicts of both kinds occur
    on every face axis."""
    n, k = 32, 60_000
    for sun in SUNS:
        ok_sun, neg, step, S, rcp = sun_consts(sun)
        assert ok_sun == 1
        assert np.array_equal(step > 0, S > 0) and np.array_equal(neg != 0, ~(S > 0))   # the walk's spelling of the signs
        X, cell, D0, fa, e = cases(n, k)
        d0a = D0[np.arange(k), fa]            # the lit term's select of D_a, handed over
        ok_o, ed_o = cert_start_old(X, D0, S, rcp, fa, e, cell)
        sig_o = walk_planes_old(X, rcp, cell, step)
        ok_n, ed_n, sig_n = cert_start_sun(X, D0, d0a, step, rcp, fa, e, cell)
        assert np.array_equal(ok_o, ok_n)
        assert np.array_equal(bits(ed_o), bits(ed_n))
        assert np.array_equal(bits(sig_o), bits(sig_n))
        for a in range(3):
            assert ok_o[fa == a].any() and (~ok_o[fa == a]).any(), (sun, a)


def test_start_predicate_truth_table():
    """fa == b || (w && f && g) on three axes, ANDed, against the integer form: all 3 * 2^9 combinations."""
    for fa in range(3):
        for v in itertools.product([False, True], repeat=9):
            old = all((fa == b) or (v[3 * b] and v[3 * b + 1] and v[3 * b + 2]) for b in range(3))
            new = 1
            for b in range(3):
                new &= int(fa == b) | (int(v[3 * b]) & int(v[3 * b + 1]) & int(v[3 * b + 2]))
            assert old == (new != 0), (fa, v)


def walk_parameters():
    """Values the primary walk's parameter can take (never negative: +0, denormals, planes' parameters) and -0."""
    u = np.concatenate([RNG.uniform(0, 400, 200_000).astype(np.float32),
                        f32(np.array([0x00000000, 0x00000001, 0x00800000, 0x3F800000, 0x7F7FFFFF], np.uint32))])
    return u


def test_record_len_is_the_parameter():
    """cert_hit_record's len = ray.len + u with ray.len = 0 is u itself for every u >= +0; -0, which the walk
    cannot produce (cert_hit_record_primary), is the one value the identity needs excluded."""
    u = walk_parameters()
    assert np.array_equal(bits(F(0) + u), bits(u))
    nz = f32(np.array([0x80000000], np.uint32))
    assert bits(F(0) + nz)[0] != bits(nz)[0]


def test_colour_of_a_primary_hit_is_the_product():
    """mixf(+0, y, 1) = +0 * (1 - 1) + y * 1 is y bit for bit for y = (col * alpha) * brightness >= +0."""
    col = np.concatenate([np.arange(256, dtype=np.float32) / F(255), np.array([0.05, 0.5, 0.1, 0.0], np.float32)])
    alpha = np.array([0.0, 1.0, 0.5, 128.0 / 255.0], np.float32)
    bright = np.concatenate([np.array([0.3], np.float32), (F(0.3) + RNG.uniform(0, 2, 500).astype(np.float32))])
    y = ((col[:, None, None] * alpha[None, :, None]) * bright[None, None, :]).reshape(-1).astype(np.float32)
    assert not np.signbit(y).any() and (y == 0).any()
    x, a = F(0), F(1)
    mix = x * (F(1) - a) + y * a
    assert np.array_equal(bits(mix), bits(y))


def test_start_texel_is_path_texel():
    """start_texel (one unsigned maximum, the load at texel 0 of an outside cell, 0 selected) against
    path_texel (three unsigned tests, 0 for an outside cell) on every cell of [-2, n + 1]^3."""
    n, p = 6, 7
    vol = RNG.integers(1, 1 << 16, p ** 3).astype(np.uint32)
    r = np.arange(-2, n + 2)
    i, j, k = [a.reshape(-1) for a in np.meshgrid(r, r, r, indexing="ij")]
    u = lambda a: a.astype(np.int64) & 0xFFFFFFFF
    out_old = (u(i) >= n) | (u(j) >= n) | (u(k) >= n)
    idx = (k * p + j) * p + i
    old = np.where(out_old, 0, vol[np.where(out_old, 0, idx)])
    out_new = np.maximum(np.maximum(u(i), u(j)), u(k)) >= n
    new = np.where(out_new, 0, vol[np.where(out_new, 0, idx)])
    assert np.array_equal(out_old, out_new) and np.array_equal(old, new)
    assert out_old.any() and (~out_old).any()


def test_air_cell_moved_predicate():
    """((ax ^ sx) | (ay ^ sy) | (az ^ sz)) != 0 is (ax, ay, az) != (sx, sy, sz), for cells at and around the
    start cell and for the indices -1 and N a cell before a hit can take."""
    vals = np.array([-1, 0, 1, 2, 63, 64, 127, 128], np.int32)
    a = np.array(list(itertools.product(vals, repeat=3)), np.int32)
    for s in itertools.product([0, 1, 64, 127], repeat=3):
        s = np.array(s, np.int32)
        new = ((a[:, 0] ^ s[0]) | (a[:, 1] ^ s[1]) | (a[:, 2] ^ s[2])) != 0
        old = (a != s).any(axis=1)
        assert np.array_equal(old, new) and (~new).sum() == 1
