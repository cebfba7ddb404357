// vrt_diag.h — the diagnostic instruments of `make variant` builds (VRT_STAMPS, VRT_CERT_DIAG,
// VRT_CERT_TRACE, and the phase cuts of VRT_PHASE_STOP): their device globals, the one-line hooks the kernels call (all empty in the
// product library; images and counters unchanged) and their debug exports. Includes vrt_internal.h only.
#ifndef VRT_DIAG_H
#define VRT_DIAG_H

#include "vrt_internal.h"

#if (defined(VRT_STAMPS) || defined(VRT_CERT_DIAG) || defined(VRT_CERT_TRACE)) && !defined(VRT_DIAGNOSTIC_BUILD)
#error "VRT_STAMPS / VRT_CERT_DIAG / VRT_CERT_TRACE are diagnostic builds: use make variant"
#endif

// ---- VRT_PHASE_STOP=k (make variant NAME=ph<k> DEFS=-DVRT_PHASE_STOP=<k>): the certified pass cut
// short after phase k, for its per-phase instruction budget as PMC differences of consecutive builds
// (DESIGN.md §6). What a phase computed goes into the pixel's colour, so it is not dead code; images
// are meaningless. 0 launch and epilogue only, 1 + ray set-up, 2 + the primary walk's start checks and
// prologue, 3 + its loop, 4 + lit term, shadow start and the shadow walk's prologue (and the sky of
// primary misses), 5 + the shadow loop; the full build adds the colour. 6: the full pass without the sky.
// Phase 4 split (a primary hit's shadow side, cert_shade_hit<.., KAX>): 7 phase 3 + the hit record, the lit
// term, the start cell and its texel (and the sky), 8 + the shadow's start (cert_start_sun); 4 adds the air
// cell's test and the shadow walk's prologue.
#ifdef VRT_PHASE_STOP
#ifndef VRT_DIAGNOSTIC_BUILD
#error "VRT_PHASE_STOP is a diagnostic build: use make variant"
#endif
#define PHASE_STOP(k) (VRT_PHASE_STOP == (k))
#else
#define PHASE_STOP(k) false
#endif

namespace vrt {

// ---- VRT_CERT_TRACE (scripts/cert_trace.py): one pixel's certified walks, 8 floats per record ----
// CTRACE_ONLY(...): its tokens in trace builds only (Ctx::tr: this lane's pixel is the traced one)
#ifdef VRT_CERT_TRACE
__device__ float g_ctrace[1024][8];
__device__ unsigned int g_ctrace_n;
#define CTRACE_ONLY(...) __VA_ARGS__
#define CTRACE(c, a0, a1, a2, a3, a4, a5, a6, a7)                                                   \
  do {                                                                                              \
    if ((c).tr) {                                                                                   \
      const unsigned int q_ = atomicAdd(&g_ctrace_n, 1u);                                           \
      if (q_ < 1024u) {                                                                             \
        g_ctrace[q_][0] = float(a0); g_ctrace[q_][1] = float(a1); g_ctrace[q_][2] = float(a2);       \
        g_ctrace[q_][3] = float(a3); g_ctrace[q_][4] = float(a4); g_ctrace[q_][5] = float(a5);       \
        g_ctrace[q_][6] = float(a6); g_ctrace[q_][7] = float(a7);                                    \
      }                                                                                             \
    }                                                                                               \
  } while (0)
#else
#define CTRACE_ONLY(...)
#define CTRACE(c, a0, a1, a2, a3, a4, a5, a6, a7) ((void)0)
#endif

// ---- VRT_CERT_DIAG (scripts/cert_diag.py): outcome counts per pixel ----------------------------
// CERT_DIAG_ONLY(...): its tokens in these builds only (CertResult::iters, the walk's iterations)
#ifdef VRT_CERT_DIAG
__device__ unsigned long long g_cert_diag[32];
#define CERT_DIAG_ONLY(...) __VA_ARGS__
#define CERT_DIAG(i) atomicAdd(&g_cert_diag[i], 1ull)
__device__ __forceinline__ void cert_diag_iters(int slot, int it) {
  atomicAdd(&g_cert_diag[slot], (unsigned long long)it);
  int m = it;
  for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off, 64));
  uint32_t l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  if (l == 0) atomicAdd(&g_cert_diag[slot + 2], (unsigned long long)m);
}
// read and reset the outcome counts (32 x u64): vrt_debug_cert_diag
int debug_cert_diag(uint64_t* out) {  // (defined here: this header belongs to one translation unit)
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_cert_diag), 32 * 8) != hipSuccess) return VRT_ERR_DEVICE;
  static const uint64_t zero[32] = {0};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_cert_diag), zero, 32 * 8) == hipSuccess ? VRT_OK : VRT_ERR_DEVICE;
}
#else
#define CERT_DIAG_ONLY(...)
#define CERT_DIAG(i) ((void)0)
#endif

// ---- VRT_STAMPS (scripts/stamps.py, exact_stamps.py): s_memrealtime (100 MHz) stamps ------------
// The hooks are statements of the kernel bodies; the *_BEGIN hooks declare the locals the later
// hooks of the same function read (and use the file's lane_id()).
#ifdef VRT_STAMPS
constexpr int kMaxStampWaves = 1 << 18;
// render_kernel, per wave (the linear wave id): {start, end, XCC_ID << 32 | HW_ID}
__device__ unsigned long long g_stamps[kMaxStampWaves][3];
// {time after the certified attempt (all lanes reconverged), lanes that took the exact path}
__device__ unsigned long long g_stamps2[kMaxStampWaves][2];
// exact_pass_kernel, per workgroup: {start, end, XCC_ID << 32 | HW_ID, pixels | dense << 16}
__device__ unsigned long long g_stamps4[kMaxStampWaves][4];
// exact_pixel, per wave: {time after the exact primary trace, after the bounce stacks}
constexpr int kMaxStampWaves3 = 1 << 18;
__device__ unsigned long long g_stamps3[kMaxStampWaves3][2];

__device__ __forceinline__ uint32_t hw_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}
__device__ __forceinline__ uint32_t xcc_id() {
  uint32_t v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v;
}

#define STAMP_WAVE_BEGIN(wave)                                 \
  const uint32_t wave_lin = ((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kWgWaves + (wave); \
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime()
#define STAMP_WAVE_CERT(need_exact)                                                       \
  do {                                                                                    \
    const unsigned long long t_cert = __builtin_amdgcn_s_memrealtime();                   \
    const unsigned long long n_exact = __builtin_popcountll(__ballot(need_exact));        \
    if (lane_id() == 0 && wave_lin < kMaxStampWaves) {                                    \
      g_stamps2[wave_lin][0] = t_cert;                                                    \
      g_stamps2[wave_lin][1] = n_exact;                                                   \
    }                                                                                     \
  } while (0)
#define STAMP_WAVE_END()                                                                  \
  do {                                                                                    \
    const unsigned long long t_end = __builtin_amdgcn_s_memrealtime();                    \
    if (lane_id() == 0 && wave_lin < kMaxStampWaves) {                                    \
      g_stamps[wave_lin][0] = t_start;                                                    \
      g_stamps[wave_lin][1] = t_end;                                                      \
      g_stamps[wave_lin][2] = (unsigned long long)xcc_id() << 32 | hw_id();               \
    }                                                                                     \
  } while (0)
#define STAMP_PIXEL_(i)                                                                                         \
  do {                                                                                                          \
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();                                              \
    if (lane_id() == uint32_t(__builtin_amdgcn_readfirstlane(int(lane_id()))) && st_wave < kMaxStampWaves3)     \
      g_stamps3[st_wave][i] = t;                                                                                \
  } while (0)
#define STAMP_PIXEL_BEGIN()                                                  \
  const uint32_t st_wave = blockIdx.x * kWgWaves + (threadIdx.x >> 6);       \
  STAMP_PIXEL_(0)
#define STAMP_PIXEL_END() STAMP_PIXEL_(1)
#define STAMP_PASS_BEGIN()                                             \
  const unsigned long long xt0 = __builtin_amdgcn_s_memrealtime();     \
  uint32_t xlanes = 0
#define STAMP_PASS_BATCH(dense) xlanes += uint32_t(__builtin_popcountll(__ballot(true))) | ((dense) ? 0x10000u : 0u)
#define STAMP_PASS_END(lane)                                                              \
  do {                                                                                    \
    const unsigned long long xt1 = __builtin_amdgcn_s_memrealtime();                      \
    if ((lane) == 0 && blockIdx.x < uint32_t(kMaxStampWaves)) {                           \
      g_stamps4[blockIdx.x][0] = xt0;                                                     \
      g_stamps4[blockIdx.x][1] = xt1;                                                     \
      g_stamps4[blockIdx.x][2] = (unsigned long long)xcc_id() << 32 | hw_id();            \
      g_stamps4[blockIdx.x][3] = xlanes;                                                  \
    }                                                                                     \
  } while (0)
#else
#define STAMP_WAVE_BEGIN(wave) ((void)0)
#define STAMP_WAVE_CERT(need_exact) ((void)0)
#define STAMP_WAVE_END() ((void)0)
#define STAMP_PIXEL_BEGIN() ((void)0)
#define STAMP_PIXEL_END() ((void)0)
#define STAMP_PASS_BEGIN() ((void)0)
#define STAMP_PASS_BATCH(dense) ((void)0)
#define STAMP_PASS_END(lane) ((void)0)
#endif

}  // namespace vrt

// ---- debug exports (diagnostic builds only; scripts/ load them from the variant library) --------
#if defined(VRT_STAMPS) || defined(VRT_CERT_DIAG) || defined(VRT_CERT_TRACE)
extern "C" {
#ifdef VRT_STAMPS
// copy the per-wave stamps of the last render (count = 3 x waves)
int vrt_debug_stamps(uint64_t* out, uint64_t count) {
  if (!out || count > 3ull * vrt::kMaxStampWaves) return VRT_ERR_INVALID;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(vrt::g_stamps), count * 8) == hipSuccess ? VRT_OK
                                                                                     : VRT_ERR_DEVICE;
}
int vrt_debug_stamps2(uint64_t* out, uint64_t count) {
  if (!out || count > 2ull * vrt::kMaxStampWaves) return VRT_ERR_INVALID;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(vrt::g_stamps2), count * 8) == hipSuccess ? VRT_OK
                                                                                     : VRT_ERR_DEVICE;
}
int vrt_debug_stamps4(uint64_t* out, uint64_t count) {
  if (!out || count > 4ull * vrt::kMaxStampWaves) return VRT_ERR_INVALID;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(vrt::g_stamps4), count * 8) == hipSuccess ? VRT_OK
                                                                                     : VRT_ERR_DEVICE;
}
int vrt_debug_stamps3(uint64_t* out, uint64_t count) {
  if (!out || count > 2ull * vrt::kMaxStampWaves) return VRT_ERR_INVALID;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(vrt::g_stamps3), count * 8) == hipSuccess ? VRT_OK
                                                                                     : VRT_ERR_DEVICE;
}
#endif
#ifdef VRT_CERT_DIAG
int vrt_debug_cert_diag(uint64_t* out) { return out ? vrt::debug_cert_diag(out) : VRT_ERR_INVALID; }
#endif
#ifdef VRT_CERT_TRACE
// the traced pixel's records (1024 x 8 floats) and their count; resets them
int vrt_debug_cert_trace(float* out, uint32_t* count) {
  if (hipDeviceSynchronize() != hipSuccess) return VRT_ERR_DEVICE;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(vrt::g_ctrace), 1024 * 8 * 4) != hipSuccess) return VRT_ERR_DEVICE;
  if (hipMemcpyFromSymbol(count, HIP_SYMBOL(vrt::g_ctrace_n), 4) != hipSuccess) return VRT_ERR_DEVICE;
  const uint32_t z = 0;
  return hipMemcpyToSymbol(HIP_SYMBOL(vrt::g_ctrace_n), &z, 4) == hipSuccess ? VRT_OK : VRT_ERR_DEVICE;
}
#endif
}  // extern "C"
#endif

#endif  // VRT_DIAG_H
