"""CPU: the certified walk's rounding bound in its factored form (vrt_cert.h cert_walk: gam_b(u) =
A(u) + |1/d_b| B(u) + ed_b, the jump test min_b(fma(fg1 - B, |1/d_b|, sig_b) - ed_b) - A without a
test of G) restated in NumPy float32 beside the per-axis form it replaces ((q2 u + q1_b) u + q0_b,
the jump test min_b(l_b - gam_b) under G >= 2), and beside the bound itself in float64 with 2^-24
where the kernel has k24 = 2 * 2^-24 (the safety factor the float evaluation must not use up).

An fma is the float64 product and sum rounded to float32: the product of two float32 is exact in
float64, the sum is rounded twice; the second rounding can move a result by one float32 ulp in
rare cases, far inside every margin asserted here.

Inputs: |d|_1 in [1, sqrt 3]; |1/d_b| from 1 up to 2^64 (the largest fast_path_ok admits), with the
smallest of the three at most sqrt 3 (a unit direction has a component >= 1 / sqrt 3); len0b in
[0, 400]; e0, ed_b in [0, 4e-3] (and exactly 0: the primary walk's instance does not add ed); N in
{16, 128, 1024}; u from 0 to the volume diagonal times the smallest |1/d_b|; G in 0..128; sig_b
within 400 |1/d_b|. Random draws, then the corners of those ranges."""
import numpy as np
import pytest

F = np.float32
K24 = F(2.0) * F(2.0 ** -24)
MARGIN = F(1.0 / 64.0)
M = 200_000


def fma(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def rcp(x):  # v_rcp_f32 within 1 ulp: the correctly rounded quotient, one ulp up and one down
    r = (F(1.0) / x).astype(F)
    return r, np.nextafter(r, F(np.inf)), np.nextafter(r, F(0.0))


def draw(n, seed):
    """A dict of float32 arrays [M] (per axis: [3, M]) over the ranges above."""
    rng = np.random.default_rng(seed)
    d = {}
    d["l1"] = rng.uniform(1.0, np.sqrt(3.0), M).astype(F)
    ar = np.exp2(rng.uniform(0.0, 64.0, (3, M)))
    ar[:, : M // 4] = np.exp2(rng.uniform(0.0, 4.0, (3, M // 4)))       # ordinary directions
    lo = rng.integers(0, 3, M)
    ar[lo, np.arange(M)] = rng.uniform(1.0, np.sqrt(3.0), M)              # the dominant axis
    d["len0b"] = rng.uniform(0.0, 400.0, M).astype(F)
    d["e0"] = rng.uniform(0.0, 4e-3, M).astype(F)
    ed = rng.uniform(0.0, 4e-3, (3, M))
    ed[:, rng.random(M) < 0.3] = 0.0
    frac = rng.random(M)
    G = rng.integers(0, 129, M)
    sfrac = rng.random((3, M))
    # corners: every range's ends, crossed
    k = 0
    for l1 in (1.0, np.sqrt(3.0)):
        for big in (1.0, 2.0 ** 64):
            for len0 in (0.0, 400.0):
                for e in (0.0, 4e-3):
                    for fr in (0.0, 1.0):
                        for g in (0, 1, 2, 128):
                            for sf in (0.0, 1.0):
                                d["l1"][k] = l1
                                ar[:, k] = (1.0, big, big if k % 2 else np.sqrt(3.0))
                                d["len0b"][k] = len0
                                d["e0"][k] = e
                                ed[:, k] = e
                                frac[k] = fr
                                G[k] = g
                                sfrac[:, k] = (sf, 1.0 - sf, sf)
                                k += 1
    d["ar"] = ar.astype(F)
    d["ed"] = ed.astype(F)
    d["fn"] = F(n)
    d["u"] = (frac * np.sqrt(3.0) * n * ar.min(axis=0)).astype(F)
    d["G"] = G.astype(np.uint32)
    d["sig"] = (sfrac * 400.0 * ar).astype(F)
    d["U"] = rng.uniform(-10.0, 300.0, M).astype(F)
    return d


def setup(d, r):
    """The walk's set-up, shared by both forms: q2, lin, con, c0 (r: the reciprocal of |d|_1 used)."""
    l1, len0b, e0 = d["l1"], d["len0b"], d["e0"]
    q2 = F(0.5) * K24 * l1
    lin = F(6.0) + l1 * (len0b + F(1.0))
    con = (F(18.0) * F(1.0000020)) * r + F(3.0) * (len0b + F(1.0))
    c0 = K24 * (con + F(2.0) * len0b) + F(4e-5) + e0
    return q2, lin, con, c0


def old_gam(d, r, u):
    q2, lin, con, c0 = setup(d, r)
    nterm = F(3.0) * d["fn"] + F(11.0)
    q1 = K24 * (lin + F(2.0) + d["ar"] * d["l1"])
    q0 = c0 + K24 * d["ar"] * nterm + d["ed"]
    return fma(fma(q2, u, q1), u, q0)


def new_AB(d, r, u):
    q2, lin, con, c0 = setup(d, r)
    a1 = K24 * (lin + F(2.0))
    b1 = K24 * d["l1"]
    b0 = K24 * (F(3.0) * d["fn"] + F(11.0))
    return fma(fma(q2, u, a1), u, c0), fma(b1, u, b0)


def new_gam(d, r, u, with_ed):
    A, B = new_AB(d, r, u)
    g = fma(B, d["ar"], A)
    return g + d["ed"] if with_ed else g


def real_bound(d, u):
    """gam_b(u) of the comment above cert_walk in float64, 2^-24 for k24, the exact 18 / |d|_1."""
    l1, len0, e0 = (d[k].astype(np.float64) for k in ("l1", "len0b", "e0"))
    ar, ed, u = d["ar"].astype(np.float64), d["ed"].astype(np.float64), u.astype(np.float64)
    n = float(d["fn"])
    K = u * l1 + 3.0
    slen = (K + 3.0) ** 2 / (2.0 * l1) + K * (len0 + 1.0)
    return 2.0 ** -24 * (slen + 2.0 * (u + len0) + (K + 3.0 * n + 8.0) * ar) + 4e-5 + e0 + ed


@pytest.fixture(scope="module", params=[16, 128, 1024])
def inputs(request):
    return draw(request.param, 20268 + request.param)


def test_factored_bound_keeps_the_safety_factor_and_the_old_value(inputs):
    d = inputs
    worst = 0.0
    for r in rcp(d["l1"]):
        old = old_gam(d, r, d["u"])
        for with_ed in (True, False):
            if not with_ed:
                d = dict(d, ed=np.zeros_like(d["ed"]))
                old = old_gam(d, r, d["u"])
            new = new_gam(d, r, d["u"], with_ed)
            assert np.all(np.isfinite(new)) and np.all(np.isfinite(old))
            R = real_bound(d, d["u"])
            assert np.all(new.astype(np.float64) >= R)
            assert np.all(new > 0) and np.all(new_AB(d, r, d["u"])[0] > 0) and np.all(new_AB(d, r, d["u"])[1] > 0)
            rel = np.abs(new.astype(np.float64) - old.astype(np.float64)) / old.astype(np.float64)
            worst = max(worst, float(rel.max()))
            assert np.all(rel <= 2.0 ** -20)
            # the factor itself: the float value stays near twice the k24 part of the bound
            k_part = R - (4e-5 + d["e0"].astype(np.float64) + d["ed"].astype(np.float64))
            assert np.all(new.astype(np.float64) - R >= 0.99 * k_part)
        d = inputs
    print(f"N {int(d['fn'])}: factored vs per-axis form, worst relative difference {worst / 2.0 ** -24:.2f} x 2^-24")


def jump_parameter(d, r, with_ed):
    """The new jump test's parameter before the length cap, and after it; u = max(s1, 0)."""
    s1 = np.minimum(d["sig"][0], np.minimum(d["sig"][1], d["sig"][2]))
    uu = np.maximum(s1, F(0.0))
    A, B = new_AB(d, r, uu)
    fg1 = d["G"].astype(F) - (F(1.0) + MARGIN)
    fb = fg1 - B
    j = fma(fb, d["ar"], d["sig"])
    if with_ed:
        j = j - d["ed"]
    jm = np.minimum(j[0], np.minimum(j[1], j[2]))
    return s1, uu, jm - A, np.minimum(jm - A, d["U"] + F(2.0))


def test_no_box_never_jumps(inputs):
    """G in {0, 1} (0: a cell outside the volume or beside a solid one; 1 also the start texel's + 1
    over a 0): the flat test's parameter is at most s1, so `uj > s1` is false without a test of G."""
    for g in (0, 1):
        d = dict(inputs, G=np.full(M, g, np.uint32))
        for r in rcp(d["l1"]):
            for with_ed in (True, False):
                dd = d if with_ed else dict(d, ed=np.zeros_like(d["ed"]))
                s1, _, raw, uj = jump_parameter(dd, r, with_ed)
                assert np.all(raw <= s1) and np.all(uj <= s1)
                assert not np.any(uj > s1)


def test_jump_lands_half_the_margin_inside_the_far_face(inputs):
    """G >= 2: uj <= min_b(sig_b + (G - 1 - 1/128) |1/d_b| - R_b) in float64, R_b the float64 bound:
    the float evaluation uses up less than half of kCertMargin (1/64 cell) and none of R_b."""
    d = dict(inputs)
    d["G"] = np.maximum(d["G"], 2).astype(np.uint32)
    d["G"][: M // 8] = 2
    d["G"][M // 8: M // 4] = 128
    for r in rcp(d["l1"]):
        for with_ed in (True, False):
            dd = d if with_ed else dict(d, ed=np.zeros_like(d["ed"]))
            s1, uu, raw, uj = jump_parameter(dd, r, with_ed)
            R = real_bound(dd, uu)
            far = dd["sig"].astype(np.float64) + (dd["G"].astype(np.float64) - 1.0 - 1.0 / 128.0) * \
                dd["ar"].astype(np.float64) - R
            lim = far.min(axis=0)
            assert np.all(raw.astype(np.float64) <= lim) and np.all(uj.astype(np.float64) <= lim)
            assert np.any(uj > s1) and np.any(~(uj > s1))   # both outcomes occur
