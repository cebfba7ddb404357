"""GPU: the two facts about powers that the certified pass's once-per-pixel cuts rest on, over all 2^32 float
bit patterns x (vrt_debug_pow_forms):
(a) the skybox's sun disc 10 * pow(x, 400), by the library's log2 and exp2 as apply_sky_color evaluates it, is
    +0 for every x in [-0, 0.75] and a NaN for every x < 0 and every NaN: a wave of primary misses none of
    which looks within 41 degrees of the sun sets it without the log and the exp;
(b) the specular power pow(max(x, 0), 10) by the bare v_log_f32 / v_exp_f32 (gpow_raw, vrt_math.h) has the
    library form's bits, or both are below 2^-100 in magnitude, where 0.2 times either vanishes in the sum
    with the ambient and diffuse terms (>= 0.3). No exception is allowed."""
import ctypes as C

import pytest

import voxelraytracer_amd as vrt

pytestmark = pytest.mark.gpu


def test_pow_forms_exhaustive(built):
    with vrt.Renderer(0) as r:
        out = (C.c_uint64 * 6)()
        r._check(r._lib.vrt_debug_pow_forms(r._h, out), "vrt_debug_pow_forms")
    far, far_bad, neg, neg_bad, spec_bad, first = list(out)
    print(f"sun disc: {far} patterns in [-0, 0.75], {far_bad} not +0; {neg} patterns negative or NaN, "
          f"{neg_bad} not NaN; specular power: {spec_bad} patterns differ at or above 2^-100"
          f"{'' if spec_bad == 0 else f', first 0x{first:08x}'}")
    # [+0, 0.75] is every pattern from 0 to 0x3f400000, and -0 one more
    assert far == 0x3F400000 + 2
    assert far_bad == 0
    # the sign bit set, but for -0; and the positive NaNs
    assert neg == (1 << 31) - 1 + ((1 << 23) - 1)
    assert neg_bad == 0
    assert spec_bad == 0, f"first pattern 0x{first:08x}"
