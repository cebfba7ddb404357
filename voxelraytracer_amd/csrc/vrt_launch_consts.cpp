// vrt_launch_consts.cpp — the launch proofs: the kernel argument block's constants that the host forms once per
// launch in place of every wave (KArgs::sun_*, fw .. max_len2, vdiv_ok, setup .. start_cell), and their test
// hooks. Every float operation here is part of the bit-exactness contract with the kernels: this file is
// built without contraction (-ffp-contract=off, as the whole library). Arithmetic only: it calls nothing of
// the HIP or RCCL runtime and includes vrt_internal.h for KArgs alone, which a plain host compiler takes
// (g++ -D__HIP_PLATFORM_AMD__ with the ROCm include path), so it also builds and links without either library.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "vrt.h"
#include "vrt_internal.h"

// normalize(u_SunDir) exactly as the kernel's normalize3 (IEEE single ops, no contraction), and its reciprocals
void vrt::fill_sun(KArgs& a, const float* sun_dir) {
  const float sx = sun_dir[0], sy = sun_dir[1], sz = sun_dir[2];
  const float inv = 1.0f / std::sqrt(sx * sx + sy * sy + sz * sz);
  a.sun_n[0] = sx * inv;
  a.sun_n[1] = sy * inv;
  a.sun_n[2] = sz * inv;
  for (int i = 0; i < 3; ++i) a.sun_rcp[i] = 1.0f / a.sun_n[i];
}

// The shadow walk's functions of the sun alone (KArgs::sun_*), once per launch instead of once per wave:
// the kernel's expressions (fast_path_ok, cert_walk's prologue, cert_shade_hit's octant) on the same
// floats in the same order. Only IEEE single additions, multiplications and compares: this file is built
// without contraction, so each value is the kernel's bit for bit (the reciprocal of l1 stays there).
void vrt::sun_consts(KArgs& a) {
  const float* s = a.sun_n;
  const float lo = 0x1p-64f, hi = 1.0e4f;
  bool ok = true;
  for (int b = 0; b < 3; ++b) ok = ok && std::fabs(s[b]) >= lo && std::fabs(s[b]) <= hi;
  a.sun_ok = ok ? 1u : 0u;
  for (int b = 0; b < 3; ++b) {
    a.sun_neg[b] = s[b] > 0.0f ? 0u : 0x80000000u;
    a.sun_step[b] = s[b] > 0.0f ? 1 : -1;
  }
  a.sun_obase = ((s[0] < 0.0f ? 1u : 0u) | (s[1] < 0.0f ? 2u : 0u) | (s[2] < 0.0f ? 4u : 0u)) * a.ostride;
  constexpr float k24 = 2.0f * 0x1p-24f;
  const float l1 = std::fabs(s[0]) + std::fabs(s[1]) + std::fabs(s[2]);
  a.sun_l1 = l1;
  a.sun_q2 = 0.5f * k24 * l1;
  a.sun_b1 = k24 * l1;
  a.sun_g2 = 2.0f * a.sun_q2;
}

// The certified pass's wave-uniform float work (KArgs::fw .. max_len2): the kernel's expressions in IEEE
// single, in its order (primary_ray's float(width), float(height) and fn * 0.5; cert_walk's b0; the primary
// walk's U + 2 with U = max_len - 0).
void vrt::setup_consts(KArgs& a) {
  constexpr float k24 = 2.0f * 0x1p-24f;
  a.fw = float(a.width);
  a.fh = float(a.height);
  a.half_n = a.fn * 0.5f;
  a.walk_b0 = k24 * (3.0f * a.fn + 11.0f);
  a.max_len2 = a.max_len + 2.0f;
}

// Per-launch proofs about the camera for the certified pass's ray set-up and walk start (KArgs::setup and
// the constants behind its flags). primary_ray forms, per pixel, n4, f4 = inv_pv^T (ndx, ndy, -+1, 1) in
// float with |ndx|, |ndy| <= 1 (a correctly rounded quotient in [0, 2], minus 1), vnear = n4.xyz / n4.w,
// vdir = f4.xyz / f4.w - vnear, P = vnear + fn / 2. Everything here is double arithmetic on the matrix,
// over the whole NDC square whatever band the launch renders, with explicit slack for the kernel's float
// evaluation; any comparison with a non-finite value fails and leaves its flag clear. A frame batch gets
// flags only when every frame's matrix is frame 0's bit for bit (the constants are the launch's).
//
// kSetupW. n4.w = ((m3 ndx + m7 ndy) + -m11) + m15. |m3 ndx + m7 ndy| <= (|m3| + |m7|)(1 + 2^-22) in
// float; if that is below ulp(m11) / 4 (ulp: the spacing of floats above |m11|, m11 normal), the sum with
// -+m11 rounds to -+m11: the nearest other float is ulp / 2 away (below a power of two), so a quarter ulp
// is under half the gap on either side and no tie can occur. Then n4.w = RN(-m11 + m15) = wn and f4.w =
// RN(m11 + m15) = wf for every pixel: formed here in IEEE single, with their reciprocals 1.0f / w
// (rcp_newton is that division on every Markstein-safe w, vrt_math.h) and the kernel's range test of d.
// Needs vdiv_ok (the numerators' upper bounds).
//
// With w constant, vnear_b = (m_b ndx + m_{4+b} ndy - m_{8+b} + m_{12+b}) / wn and the far point likewise
// are affine in (ndx, ndy). Float evaluation: a numerator is within 2^-21 S_b of the real one (S_b = the
// column's absolute sum: four products, three sums), the quotient rounds once more: within en_b = 2^-19
// S_b / |wn| of the real affine value, ef_b likewise; vdir_b within ev_b = 2 (en_b + ef_b).
//
// kSetupLen. normalize3(vdir) takes rcp_newton(sqrt_fix(s)) unguarded when s = |vdir|^2 is outside the
// near-one window (|s - 1| > 2^-13), in [2^-32, 2^126) and its root in [2^-125, 2^126). Lower bound of
// |vdir|: its projection on the centre pixel's direction c / |c|, an affine function, so its minimum over
// the square is at a corner: |c| - |a . c| / |c| - |b . c| / |c|, minus |ev|_1. Upper bound: |vfar|_1 +
// |vnear|_1 <= sum_b S_b (1 / |wf| + 1 / |wn|), plus |ev|_1. Held to [4, 2^49]: s in [16, 2^98] up to the
// float evaluation's relative 2^-21, orders of magnitude inside every threshold.
//
// kSetupCell. P_b ranges over centre +- spread with centre = (-m_{8+b} + m_{12+b}) / wn + fn / 2 and
// spread = (|m_b| + |m_{4+b}|) / |wn|; the kernel's P_b is within en_b + 2^-23 (|centre| + spread) of it
// (the sum's rounding). With a further 2^-9 on both sides the interval must lie strictly inside one cell
// (c_b, c_b + 1), 0 <= c_b < N: then floor(P_b) = c_b, P_b is no integer, and the start's plane tests
// hold with room for their own rounding (cert_pixel).
void vrt::cert_launch_consts(KArgs& a) {
  a.setup = 0u;
  a.wn = a.wf = a.rcp_wn = a.rcp_wf = 0.0f;
  for (int i = 0; i < 6; ++i) a.start_fl1[i] = 0.0f;
  for (int b = 0; b < 3; ++b) a.start_cell[b] = 0;
  if (a.vdiv_ok == 0u) return;
  for (int f = 1; f < a.nframes; ++f)
    if (std::memcmp(a.fb[f - 1].inv_pv, a.inv_pv, sizeof(a.inv_pv)) != 0) return;
  const float* m = a.inv_pv;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(m[i])) return;

  // ---- w constant
  const double am11 = std::fabs(double(m[11]));
  if (!(am11 >= double(std::numeric_limits<float>::min()))) return;  // normal (and not zero)
  const double ulp = std::ldexp(1.0, std::ilogb(am11) - 23);
  if (!((std::fabs(double(m[3])) + std::fabs(double(m[7]))) * (1.0 + 0x1p-20) < ulp * 0.25)) return;
  const float wn = -m[11] + m[15], wf = m[11] + m[15];
  const auto markstein = [](float x) { return std::fabs(x) >= 0x1p-60f && std::fabs(x) <= 0x1p60f; };
  if (!markstein(wn) || !markstein(wf)) return;
  a.wn = wn;
  a.wf = wf;
  a.rcp_wn = 1.0f / wn;
  a.rcp_wf = 1.0f / wf;
  a.setup |= kSetupW;

  // ---- the affine near and far points
  const double iwn = 1.0 / std::fabs(double(wn)), iwf = 1.0 / std::fabs(double(wf));
  double S[3], en[3], ev1 = 0.0, up = 0.0;
  double ca[3], cb[3], cc[3];  // vdir = ca ndx + cb ndy + cc
  for (int b = 0; b < 3; ++b) {
    S[b] = std::fabs(double(m[b])) + std::fabs(double(m[4 + b])) + std::fabs(double(m[8 + b])) +
           std::fabs(double(m[12 + b]));
    en[b] = 0x1p-19 * S[b] * iwn;
    const double ef = 0x1p-19 * S[b] * iwf;
    ev1 += 2.0 * (en[b] + ef);
    up += S[b] * (iwn + iwf);
    const double d = 1.0 / double(wf) - 1.0 / double(wn);
    ca[b] = double(m[b]) * d;
    cb[b] = double(m[4 + b]) * d;
    cc[b] = (double(m[8 + b]) + double(m[12 + b])) / double(wf) - (double(m[12 + b]) - double(m[8 + b])) / double(wn);
  }

  // ---- squared length of vdir
  const double cl = std::sqrt(cc[0] * cc[0] + cc[1] * cc[1] + cc[2] * cc[2]);
  if (cl > 0.0 && std::isfinite(cl)) {
    const double pa = std::fabs(ca[0] * cc[0] + ca[1] * cc[1] + ca[2] * cc[2]) / cl;
    const double pb = std::fabs(cb[0] * cc[0] + cb[1] * cc[1] + cb[2] * cc[2]) / cl;
    // (the double evaluation itself: relative 2^-50 of sums of the terms' magnitudes, far inside 2^-19 S / |w|)
    if (cl - pa - pb - ev1 >= 4.0 && up + ev1 <= 0x1p49) a.setup |= kSetupLen;
  }

  // ---- start cell
  const double half = double(a.fn) * 0.5;
  int32_t cell[3];
  for (int b = 0; b < 3; ++b) {
    const double centre = (double(m[12 + b]) - double(m[8 + b])) / double(wn) + half;
    const double spread = (std::fabs(double(m[b])) + std::fabs(double(m[4 + b]))) * iwn;
    const double e = en[b] + 0x1p-23 * (std::fabs(centre) + half + spread) + 0x1p-9;
    const double lo = centre - spread - e, hi = centre + spread + e;
    const double c = std::floor(lo);
    if (!(lo > c && hi < c + 1.0 && c >= 0.0 && c < double(a.n))) return;
    cell[b] = int32_t(c);
  }
  for (int b = 0; b < 3; ++b) {
    a.start_cell[b] = cell[b];
    a.start_fl1[b] = float(cell[b] + 1);
    a.start_fl1[3 + b] = float(-cell[b]);
  }
  a.setup |= kSetupCell;
}

// The vertex stage's divisions (primary_ray: n4.xyz / n4.w and f4.xyz / f4.w, with n4, f4 =
// inv_pv^T (ndx, ndy, -+1, 1)) take Markstein's sequence when every operand's magnitude is in
// [2^-60, 2^60]. All but the numerators' lower bound follows from the matrix, since |ndx|, |ndy| <=
// 1 (a correctly rounded quotient in [0, 2], minus 1): component i is at most S_i = |m_0i| + |m_1i|
// + |m_2i| + |m_3i| in magnitude, and the denominators are at least |m_33 -+ m_23| - |m_03| -
// |m_13|. The kernel forms them in float, four products and three sums: within 2^-21 S_i of the
// real value, allowed for here as 2^-20 S_i, and the bounds are held to 2^59 and 2^-59, one binade
// inside the kernel's. true: every pixel's operands pass all of the kernel's tests except
// "|numerator| >= 2^-60" (NaN or infinite entries: false).
bool vrt::vertex_div_ranges_ok(const float* m) {
  const double hi = 0x1p59, lo = 0x1p-59;
  double sum[4];
  for (int i = 0; i < 4; ++i) {
    sum[i] = std::fabs(double(m[i])) + std::fabs(double(m[4 + i])) + std::fabs(double(m[8 + i])) +
             std::fabs(double(m[12 + i]));
    if (!(sum[i] * (1.0 + 0x1p-20) <= hi)) return false;
  }
  const double side = std::fabs(double(m[3])) + std::fabs(double(m[7])) + sum[3] * 0x1p-20;
  return std::fabs(double(m[15]) - double(m[11])) - side >= lo &&  // n4.w
         std::fabs(double(m[15]) + double(m[11])) - side >= lo;    // f4.w
}

extern "C" {

// Test hook, not part of vrt.h (tests/test_cert_start_lit_forms.py): the twelve KArgs::sun_* words, in
// the struct's order, for normalize(sun_dir) as make_args forms it. Host arithmetic only, no device.
int vrt_debug_sun_consts(const float* sun_dir, uint32_t ostride, uint32_t* out) {
  if (!sun_dir || !out) return VRT_ERR_INVALID;
  vrt::KArgs a{};
  vrt::fill_sun(a, sun_dir);
  a.ostride = ostride;
  vrt::sun_consts(a);
  std::memcpy(out, &a.sun_ok, 12 * sizeof(uint32_t));
  return VRT_OK;
}

// Test hook, not part of vrt.h (tests/test_cert_launch_consts.py): the certified pass's launch constants as
// launch() fills them for the camera matrix inv_pv (and, with inv_pv2, for a two-frame batch of both), an N^3
// volume and a width x height frame. Host arithmetic only, no device. out[0..18]: KArgs::setup, wn, wf,
// rcp_wn, rcp_wf, start_fl1[6], start_cell[3], fw, fh, half_n, walk_b0, max_len2; out[19]: vdiv_ok.
int vrt_debug_cert_launch_consts(const float* inv_pv, const float* inv_pv2, int32_t n, int32_t width, int32_t height,
                                 float max_len, uint32_t* out) {
  if (!inv_pv || !out) return VRT_ERR_INVALID;
  vrt::KArgs a{};
  std::memcpy(a.inv_pv, inv_pv, sizeof(a.inv_pv));
  a.n = n;
  a.fn = float(n);
  a.width = width;
  a.height = height;
  a.max_len = max_len;
  a.nframes = 1;
  a.vdiv_ok = vrt::vertex_div_ranges_ok(a.inv_pv) ? 1u : 0u;
  if (inv_pv2) {
    a.nframes = 2;
    std::memcpy(a.fb[0].inv_pv, inv_pv2, sizeof(a.inv_pv));
    if (!vrt::vertex_div_ranges_ok(a.fb[0].inv_pv)) a.vdiv_ok = 0u;
  }
  vrt::setup_consts(a);
  vrt::cert_launch_consts(a);
  out[0] = a.setup;
  std::memcpy(out + 1, &a.wn, 4 * sizeof(float));
  std::memcpy(out + 5, a.start_fl1, 6 * sizeof(float));
  std::memcpy(out + 11, a.start_cell, 3 * sizeof(int32_t));
  std::memcpy(out + 14, &a.fw, 5 * sizeof(float));
  out[19] = a.vdiv_ok;
  return VRT_OK;
}

}  // extern "C"
