// vrt_aux_kernels.h — the kernels beside the frame: glass share, scene build, band assembly, RGB8 pack,
// randomize, counter reduce, the fast-math check. (The skip field of the packed volume is built by
// vrt_skipfield_kernels.h.) Includes vrt_internal.h, vrt_math.h and vrt_walk.h.
#ifndef VRT_AUX_KERNELS_H
#define VRT_AUX_KERNELS_H

#include "vrt_internal.h"
#include "vrt_math.h"
#include "vrt_walk.h"

namespace vrt {

// Glass and non-empty voxel counts of the canonical volume (vrt_set_certified's automatic mode):
// one wave-reduced atomic pair per wave.
__global__ void __launch_bounds__(256) glass_share_kernel(const uint8_t* __restrict__ vox, uint64_t total,
                                                          unsigned long long* __restrict__ out) {
  unsigned long long g = 0, ne = 0;
  for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += uint64_t(gridDim.x) * 256) {
    const uint32_t b = vox[i];
    ne += b != 0u ? 1ull : 0ull;
    g += mat_id(b) == 2u ? 1ull : 0ull;
  }
  for (int off = 32; off > 0; off >>= 1) {
    g += __shfl_xor(g, off, 64);
    ne += __shfl_xor(ne, off, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (g) atomicAdd(out, g);
    if (ne) atomicAdd(out + 1, ne);
  }
}

// Scene builders of main.cpp:218-288 on the device (vrt_build_scene_device): one work-item per
// voxel applies the host builders' writes in their order (csrc/vrt_host.cpp vrt_build_scene);
// `noise` is the n*n terrain heightfield (x + z*n), only read for _TERRAIN.
__global__ void __launch_bounds__(256) build_scene_kernel(uint8_t* __restrict__ vox, int scene,
                                                          uint32_t n, const float* __restrict__ noise) {
  const uint64_t total = uint64_t(n) * n * n;
  const float fs = float(n);
  const uint32_t lo = n / 4, hi = 3 * n / 4, c = n / 2;
  for (uint64_t idx = uint64_t(blockIdx.x) * 256 + threadIdx.x; idx < total;
       idx += uint64_t(gridDim.x) * 256) {
    const uint32_t x = uint32_t(idx % n), y = uint32_t((idx / n) % n), z = uint32_t(idx / (uint64_t(n) * n));
    uint8_t v = 0;
    if (scene == VRT_SCENE_TERRAIN) {  // main.cpp:219-257
      const float h = noise[x + z * n] * fs;
      if (float(int(y)) < h) v = 1;                     // stone column
      if (int(y) == int(h)) v = 3;                      // grass cap
      if (n <= 64) {                                    // glass walls (main.cpp:233)
        if (x == 0 && z >= 2 && z < n - 2 && int(y) >= int(noise[z * n] * fs + 1.0f)) v = 2;
        if (z == n - 4 && x >= 2 && x < n - 1 && int(y) >= int(noise[x * n + n - 4] * fs + 1.0f) &&
            int(y) < int(n) - 4)
          v = 2;
      }
      if (x == n - 1 && z >= 2 && z < n - 2 && int(y) >= int(noise[n - 1 + z * n] * fs + 1.0f) &&
          int(y) < int(n) - 4)
        v = 3;
    } else if (scene == VRT_SCENE_GLASS_CUBE) {  // main.cpp:258-271
      if (x == 0 || x == n - 1 || y == 0 || y == n - 1 || z == 0 || z == n - 1) v = 2;
      if (x == c && y == c && z == c) v = 3;
    } else {  // VRT_SCENE_REFRACTION, main.cpp:272-287
      if (x == c && y == c && z == c) v = 2;
      const bool in_yz = y >= lo && y < hi && z >= lo && z < hi;
      const bool in_xy = x >= lo && x < hi && y >= lo && y < hi;
      const bool in_xz = x >= lo && x < hi && z >= lo && z < hi;
      if (((x == 0 || x == n - 1) && in_yz) || ((z == 0 || z == n - 1) && in_xy) ||
          ((y == 0 || y == n - 1) && in_xz))
        v = 3;
    }
    vox[idx] = v;
  }
}

// Frame assembly of block-cyclic bands (ABI v12; the re-interleave after a gather of the bands to
// one device): band j of k holds the frame's row blocks j, j + k, ... of 2^sh rows, so its row i is
// frame row ((i >> sh) * k + j) * 2^sh + (i & (2^sh - 1)); bands lie band_words words apart. One
// workgroup per frame row copies the row from its band: 16-byte words when VEC (width, band_words
// and frame_pitch multiples of 4 words, 16-byte aligned buffers), else 4-byte words. HBM-bound:
// 8 B of traffic per pixel, no reuse.
template <bool VEC>
__global__ void __launch_bounds__(256) assemble_blocks_kernel(const uint32_t* __restrict__ bands,
                                                              uint64_t band_words, int32_t k, int32_t sh,
                                                              int32_t width, uint32_t* __restrict__ frame,
                                                              uint64_t frame_pitch) {
  const uint32_t y = blockIdx.x;
  const uint32_t m = y >> sh;
  const uint32_t j = m % uint32_t(k), mb = m / uint32_t(k);
  const uint64_t bi = (uint64_t(mb) << sh) + (y & ((1u << sh) - 1u));
  const uint32_t* src = bands + uint64_t(j) * band_words + bi * uint64_t(width);
  uint32_t* dst = frame + uint64_t(y) * frame_pitch;
  if (VEC) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (uint32_t x = threadIdx.x; x < uint32_t(width) / 4u; x += 256u) d4[x] = s4[x];
  } else {
    for (uint32_t x = threadIdx.x; x < uint32_t(width); x += 256u) dst[x] = src[x];
  }
}

// RGB8 wire format of a gathered band (ABI v12): the RGBA8 words' alpha byte is always 255
// (pack_rgb8), so a band crosses xGMI as 3 bytes per pixel — 25 % fewer bytes into rank 0, whose
// ingress bounds the per-frame gather. Four pixels per work-item: one 16-byte load,
// three 4-byte stores (pixels is a multiple of 4).
__global__ void __launch_bounds__(256) pack_rgb8_kernel(const uint4* __restrict__ rgba, uint64_t quads,
                                                        uint32_t* __restrict__ rgb) {
  for (uint64_t q = uint64_t(blockIdx.x) * 256 + threadIdx.x; q < quads; q += uint64_t(gridDim.x) * 256) {
    const uint4 p = rgba[q];
    const uint32_t a = p.x & 0xFFFFFFu, b = p.y & 0xFFFFFFu, c = p.z & 0xFFFFFFu, d = p.w & 0xFFFFFFu;
    // one 12-byte store per work-item (a wave writes 768 contiguous bytes per instruction)
    reinterpret_cast<uint3*>(rgb)[q] = make_uint3(a | (b << 24), (b >> 8) | (c << 16), (c >> 16) | (d << 8));
  }
}

// assemble_blocks_kernel for RGB8 bands (band_px pixels apart, 3 bytes each): each frame row from
// its band, unpacked to RGBA8 words (A = 255); four pixels per work-item (width % 4 == 0)
__global__ void __launch_bounds__(256) assemble_blocks_rgb8_kernel(const uint32_t* __restrict__ bands,
                                                                   uint64_t band_px, int32_t k, int32_t sh,
                                                                   int32_t width, uint4* __restrict__ frame,
                                                                   uint64_t frame_pitch) {
  const uint32_t y = blockIdx.x;
  const uint32_t m = y >> sh;
  const uint32_t j = m % uint32_t(k), mb = m / uint32_t(k);
  const uint64_t bi = (uint64_t(mb) << sh) + (y & ((1u << sh) - 1u));
  const uint32_t* src = bands + (uint64_t(j) * band_px + bi * uint64_t(width)) * 3u / 4u;
  uint4* dst = frame + uint64_t(y) * frame_pitch / 4u;
  for (uint32_t x = threadIdx.x; x < uint32_t(width) / 4u; x += 256u) {
    const uint3 t = reinterpret_cast<const uint3*>(src)[x];  // one 12-byte load (768 B per wave)
    const uint32_t u = t.x, v = t.y, w = t.z;
    dst[x] = make_uint4(0xFF000000u | (u & 0xFFFFFFu), 0xFF000000u | (u >> 24) | ((v & 0xFFFFu) << 8),
                        0xFF000000u | (v >> 16) | ((w & 0xFFu) << 16), 0xFF000000u | (w >> 8));
  }
}

// Diagnostic: RandomizeDirection for n (dir, pos) pairs (vrt_debug_randomize).
__global__ void __launch_bounds__(64) randomize_kernel(const float* __restrict__ dir,
                                                       const float* __restrict__ pos, int n,
                                                       float randomness, float seed,
                                                       float* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const f3 r = randomize(mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]),
                         mk(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]), randomness, seed);
  out[3 * i] = r.x;
  out[3 * i + 1] = r.y;
  out[3 * i + 2] = r.z;
}

// Sum the counter replicas into `dst` (accumulating) and zero them for the next render.
__global__ void __launch_bounds__(64) reduce_counters_kernel(unsigned long long* __restrict__ rep,
                                                             unsigned long long* __restrict__ dst) {
  const int q = threadIdx.x;
  if (q >= VRT_CNT_COUNT) return;
  unsigned long long s = 0;
  for (int r = 0; r < kCntReplicas; ++r) {
    s += rep[r * VRT_CNT_COUNT + q];
    rep[r * VRT_CNT_COUNT + q] = 0;
  }
  dst[q] += s;
}

// Diagnostic (vrt_debug_fast_math): every float bit pattern, rcp_newton against the IEEE
// division. out: {patterns with rcp_rn_ok, their mismatches, mismatches of normal-range patterns
// with an all-ones significand, mismatches of the other (non-NaN) patterns, the first mismatching
// pattern with rcp_rn_ok (or ~0); then sqrt_fix against the IEEE square root: positive patterns
// with sqrt_fix_ok, their mismatches}
__global__ void fast_math_check_kernel(unsigned long long* out) {
  const uint64_t per = 256;
  const uint64_t base = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) * per;
  uint32_t ok = 0, bad_ok = 0, bad_ones = 0, bad_other = 0, sq_ok = 0, sq_bad = 0;
  for (uint64_t i = 0; i < per; ++i) {
    const uint32_t u = uint32_t(base + i);
    const float d = __uint_as_float(u);
    const uint32_t ex = (u >> 23) & 0xFFu;
    const bool in_range = ex >= 2u && ex <= 252u;
    const bool fine = rcp_rn_ok(d);
    const bool same = __float_as_uint(rcp_newton(d)) == __float_as_uint(1.0f / d);
    ok += fine ? 1u : 0u;
    if (sqrt_fix_ok(d) && d > 0.0f) {
      ++sq_ok;
      if (__float_as_uint(sqrt_fix(d)) != __float_as_uint(__builtin_sqrtf(d))) ++sq_bad;
    }
    if (!same && !(d != d)) {
      if (fine) {
        ++bad_ok;
        atomicMin(&out[4], (unsigned long long)u);
      } else if (in_range) {
        ++bad_ones;
      } else {
        ++bad_other;
      }
    }
  }
  atomicAdd(&out[0], (unsigned long long)ok);
  atomicAdd(&out[1], (unsigned long long)bad_ok);
  atomicAdd(&out[2], (unsigned long long)bad_ones);
  atomicAdd(&out[3], (unsigned long long)bad_other);
  atomicAdd(&out[5], (unsigned long long)sq_ok);
  atomicAdd(&out[6], (unsigned long long)sq_bad);
}

// Diagnostic (vrt_debug_pow_forms): every float bit pattern x through the two powers the certified pass
// shortens. out: {(a) patterns in [-0, 0.75], those whose 10 * gpow(x, 400) (apply_sky_color's sun disc) is not
// +0, patterns with x < 0 or NaN, those whose result is no NaN; (b) patterns whose gpow and gpow_raw of
// (max(x, 0), 10) (cert_shade_hit's specular power) differ in their bits while either is a NaN or at least
// 2^-100 in magnitude, the first such pattern (or ~0)}. The values pass through opaque registers, so that the
// compiler evaluates each form as the render kernels do and folds nothing across the comparison.
__global__ void pow_forms_check_kernel(unsigned long long* out) {
  const uint64_t per = 256;
  const uint64_t base = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) * per;
  uint32_t far = 0, far_bad = 0, neg = 0, neg_bad = 0, spec_bad = 0;
  for (uint64_t i = 0; i < per; ++i) {
    const uint32_t u = uint32_t(base + i);
    float x = __uint_as_float(u);
    asm volatile("" : "+v"(x));
    const float sun = 10.0f * gpow(x, 400.0f);
    if (u == 0x80000000u || (x >= 0.0f && x <= 0.75f)) {
      ++far;
      if (__float_as_uint(sun) != 0u) ++far_bad;
    } else if (!(x >= 0.0f)) {  // x < 0 or NaN (-0 was taken above)
      ++neg;
      if (sun == sun) ++neg_bad;
    }
    float m = gmax(x, 0.0f);
    asm volatile("" : "+v"(m));
    const float lib = gpow(m, 10.0f), raw = gpow_raw(m, 10.0f);
    const bool tiny = __builtin_fabsf(lib) < 0x1p-100f && __builtin_fabsf(raw) < 0x1p-100f;  // (false for a NaN)
    if (__float_as_uint(lib) != __float_as_uint(raw) && !tiny) {
      ++spec_bad;
      atomicMin(&out[5], (unsigned long long)u);
    }
  }
  atomicAdd(&out[0], (unsigned long long)far);
  atomicAdd(&out[1], (unsigned long long)far_bad);
  atomicAdd(&out[2], (unsigned long long)neg);
  atomicAdd(&out[3], (unsigned long long)neg_bad);
  atomicAdd(&out[4], (unsigned long long)spec_bad);
}

}  // namespace vrt

#endif  // VRT_AUX_KERNELS_H
