"""CPU truth tables of the certified pass's lean forms (vrt_cert.h cert_walk<.., LEAN>, vrt_math.h
zero_noise_exact_class, vrt_render.hip div3_rn<LEAN>, vrt_launch_consts.cpp vertex_div_ranges_ok): each
lean form is restated in NumPy float32 beside the form it replaces and compared over the special
values (+-0, NaN, +-inf, denormals, the thresholds 2^-64, 2^-60, 2^60, 1e4 and their neighbours)
and a few million random bit patterns. v_min3_f32 / v_max3_f32 are np.fmin / np.fmax (a NaN operand
is dropped), v_cmp_class_f32 is a test of the operand's bits."""
import numpy as np

RNG = np.random.default_rng(20260)


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def neighbours(values):
    b = bits(np.array(values, np.float32)).astype(np.int64)
    out = np.concatenate([b - 2, b - 1, b, b + 1, b + 2]) & 0xFFFFFFFF
    return f32(out.astype(np.uint32))


SPECIAL = np.concatenate([
    neighbours([0.0, 1.0, 2.0 ** -64, 2.0 ** -60, 2.0 ** 60, 1.0e4, 2.0 ** -126, 2.0 ** -149, 3.0e38]),
    -neighbours([0.0, 1.0, 2.0 ** -64, 2.0 ** -60, 2.0 ** 60, 1.0e4, 2.0 ** -126, 2.0 ** -149, 3.0e38]),
    f32(np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF,
                  0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF], np.uint32)),
])


def triples(n_random):
    """Every triple of special values in x with y, z drawn from the specials, then random patterns."""
    s = SPECIAL
    i = RNG.integers(0, len(s), (3, 200_000))
    grid = [np.concatenate([np.repeat(s, len(s)), s[i[0]]]), np.concatenate([np.tile(s, len(s)), s[i[1]]]),
            np.concatenate([np.resize(s, len(s) * len(s)), s[i[2]]])]
    rnd = f32(RNG.integers(0, 2 ** 32, (3, n_random), dtype=np.uint64).astype(np.uint32))
    return [np.concatenate([grid[k], rnd[k]]) for k in range(3)]


def test_zero_noise_exact_class():
    """zero_noise_exact: no component is -0 (bit pattern) or NaN; the class form tests the classes
    -0, signalling NaN and quiet NaN per component."""
    x, y, z = triples(3_000_000)
    nz = np.uint32(0x80000000)
    with np.errstate(invalid="ignore"):
        old = (bits(x) != nz) & (bits(y) != nz) & (bits(z) != nz) & (x == x) & (y == y) & (z == z)

    def cls(v):  # v_cmp_class_f32 v, 0x23: by the bits alone
        b = bits(v)
        mag = b & np.uint32(0x7FFFFFFF)
        return (b == nz) | (mag > np.uint32(0x7F800000))

    new = ~(cls(x) | cls(y) | cls(z))
    assert np.array_equal(old, new)
    assert old.any() and (~old).any()


def markstein_safe(v):
    with np.errstate(invalid="ignore"):
        m = np.abs(v)
        return (m >= np.float32(2.0 ** -60)) & (m <= np.float32(2.0 ** 60))


def test_vertex_division_test_split():
    """div3_rn's test, all of |x|, |y|, |z|, |d| in [2^-60, 2^60], against its lean split: the part
    the host may prove per launch (upper bounds, the denominator's range; it rejects NaN) and the
    lane's part, min3(|x|, |y|, |z|) >= 2^-60, whose minimum drops NaN operands."""
    x, y, z = triples(2_000_000)
    d = np.concatenate([SPECIAL[RNG.integers(0, len(SPECIAL), len(x) - 1_000_000)],
                        f32(RNG.integers(0, 2 ** 32, 1_000_000, dtype=np.uint64).astype(np.uint32))])
    old = markstein_safe(x) & markstein_safe(y) & markstein_safe(z) & markstein_safe(d)
    hi = np.float32(2.0 ** 60)
    with np.errstate(invalid="ignore"):
        rest = (np.abs(x) <= hi) & (np.abs(y) <= hi) & (np.abs(z) <= hi) & markstein_safe(d)
        lane = np.fmin(np.fmin(np.abs(x), np.abs(y)), np.abs(z)) >= np.float32(2.0 ** -60)
    assert np.array_equal(old, rest & lane)
    # with the host's flag the lane's part alone decides: it must equal the full test wherever
    # `rest` holds (the flag is only set where `rest` holds for every pixel)
    assert np.array_equal(old[rest], lane[rest])
    assert old.any() and (rest & ~lane).any() and (~rest & lane).any()


def test_fast_path_ok_minmax_form_is_not_exact():
    """fast_path_ok keeps its six compares: the min3 / max3 form (two compares) drops NaN operands
    and so accepts a direction with a NaN beside two in-range components, which the compares
    reject. The forms agree on every NaN-free triple; the recorded reason the cut was left out."""
    x, y, z = triples(2_000_000)
    lo, hi = np.float32(2.0 ** -64), np.float32(1.0e4)
    with np.errstate(invalid="ignore"):
        ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
        old = (ax >= lo) & (ay >= lo) & (az >= lo) & (ax <= hi) & (ay <= hi) & (az <= hi)
        new = (np.fmin(np.fmin(ax, ay), az) >= lo) & (np.fmax(np.fmax(ax, ay), az) <= hi)
    nan = np.isnan(x) | np.isnan(y) | np.isnan(z)
    assert np.array_equal(old[~nan], new[~nan])
    assert not old[nan].any() and new[nan].any()


def test_sig_from_floored_float():
    """The next plane's parameter after a jump, ((fl + 1) - Ps) * |rcp| with the sign-folded start
    Ps = s P, against (float(c + u) - P) * rcp with c = fl (moving up, u = 1) or ~fl (moving down,
    u = 0); and after a crossing into cell index na, (float((na ^ m) + 1) - Ps) * |rcp| against
    (float(na + u) - P) * rcp. Bit for bit, zeros' signs aside: the walk's values are never zero
    there (the plane lies ahead of the start)."""
    n = 2_000_000
    fl = RNG.integers(-3, 1027, n).astype(np.int32)            # floor of the folded landing coordinate
    P = np.concatenate([RNG.uniform(-2.0, 1026.0, n - 4096).astype(np.float32),
                        RNG.integers(-2, 1026, 4096).astype(np.float32)])
    rcp_mag = f32(RNG.integers(0x2F800000, 0x5F800000, n, dtype=np.uint64).astype(np.uint32))  # 2^-32 .. 2^64
    for up in (True, False):
        u = 1 if up else 0
        m = np.int32(0 if up else -1)
        Ps = P if up else -P
        rcp = rcp_mag if up else -rcp_mag
        ar = np.abs(rcp)
        flf = fl.astype(np.float32)
        c = fl ^ m
        old = ((c + u).astype(np.float32) - P) * rcp
        new = ((flf + np.float32(1.0)) - Ps) * ar
        nonzero = old != 0
        assert np.array_equal(bits(old)[nonzero], bits(new)[nonzero])
        assert np.array_equal(old, new)  # zeros equal in value
        na = c                                                   # a crossing's new cell index
        old_c = ((na + u).astype(np.float32) - P) * rcp
        new_c = (((na ^ m) + 1).astype(np.float32) - Ps) * ar
        nonzero = old_c != 0
        assert np.array_equal(bits(old_c)[nonzero], bits(new_c)[nonzero])
        assert np.array_equal(old_c, new_c)


def test_crossing_outside_is_one_unsigned_maximum():
    """A crossing from a cell in [0, N)^3 changes one index by +-1: the unsigned maximum of the
    three new indices is >= N exactly when that index left [0, N) (-1 wraps to 2^32 - 1)."""
    for n in (2, 16, 1024):
        c = RNG.integers(0, n, (3, 100_000)).astype(np.int64)
        a = RNG.integers(0, 3, 100_000)
        s = RNG.choice(np.array([-1, 1]), 100_000)
        c[:, :64] = np.array([[0, n - 1] * 32] * 3)  # the faces and corners
        nc = c.copy()
        nc[a, np.arange(c.shape[1])] += s
        na = nc[a, np.arange(c.shape[1])]
        left = (na < 0) | (na >= n)
        mx = (nc & 0xFFFFFFFF).max(axis=0)
        assert np.array_equal(left, mx >= n)
        assert left.any() and (~left).any()
