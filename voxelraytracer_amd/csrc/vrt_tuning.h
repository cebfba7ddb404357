// vrt_tuning.h — every numeric A/B knob of the kernels and the context: its default, the
// measurement behind the default, and the constant the code names. Includes <cstdint> only (it
// preprocesses with a plain host compiler, tests/test_tuning_guard.py).
#ifndef VRT_TUNING_H
#define VRT_TUNING_H

#include <cstdint>

// The product library is built with the defaults below. Another value is an A/B build:
// make variant NAME=w6 DEFS=-DVRT_MIN_WAVES=6 (which defines VRT_DIAGNOSTIC_BUILD).
#if (defined(VRT_MIN_WAVES) || defined(VRT_DEFER_WAVES) || defined(VRT_EXACT_WAVES) || defined(VRT_TREE_WAVES) || \
     defined(VRT_FAT_WAVES) || defined(VRT_SPARSE_BATCH) || defined(VRT_SPARSE_BATCH_TEX) ||                    \
     defined(VRT_SPARSE_BATCH_FAT) || defined(VRT_EXACT_PRIO) || defined(VRT_FWD_CAP) || defined(VRT_WG_WAVES) || \
     defined(VRT_ORD_DIV) || defined(VRT_ORD_MIN_ROUNDS) || defined(VRT_DEFER_GRID_DIV) ||                      \
     defined(VRT_DEFER_GRID_DIV_COLOR) || defined(VRT_QUERY_WG_WAVES) || defined(VRT_TRACE_WG_WAVES) ||         \
     defined(VRT_TRACE_MIN_WAVES) || defined(VRT_DEFER_LDS_PAD) || defined(VRT_EXACT_VGPRS) ||                  \
     defined(VRT_SPATIAL_LDS_STEPS) || defined(VRT_NO_SKY_ZERO) || defined(VRT_NO_RAW_SPECULAR)) &&            \
    !defined(VRT_DIAGNOSTIC_BUILD)
#error "the VRT_* tuning values are A/B knobs of make variant builds (make variant NAME=... DEFS=-DVRT_...=...)"
#endif

#ifndef VRT_WG_WAVES
#define VRT_WG_WAVES 2
#endif
#ifndef VRT_MIN_WAVES  // occupancy A/B builds (make variant); images identical at any value
#define VRT_MIN_WAVES 7
#endif
#ifndef VRT_DEFER_WAVES
#define VRT_DEFER_WAVES 7
#endif
#ifndef VRT_DEFER_LDS_PAD
#define VRT_DEFER_LDS_PAD 0
#endif
#ifndef VRT_EXACT_WAVES
#define VRT_EXACT_WAVES VRT_MIN_WAVES
#endif
#ifndef VRT_EXACT_VGPRS
#define VRT_EXACT_VGPRS 120
#endif
#ifndef VRT_TREE_WAVES
#define VRT_TREE_WAVES 5
#endif
#ifndef VRT_FAT_WAVES
#define VRT_FAT_WAVES 3
#endif
#ifndef VRT_SPARSE_BATCH
#define VRT_SPARSE_BATCH 32
#endif
#ifndef VRT_SPARSE_BATCH_TEX
#define VRT_SPARSE_BATCH_TEX 64
#endif
#ifndef VRT_SPARSE_BATCH_FAT
#define VRT_SPARSE_BATCH_FAT 16
#endif
#ifndef VRT_EXACT_PRIO
#define VRT_EXACT_PRIO 2
#endif
#ifndef VRT_FWD_CAP
#define VRT_FWD_CAP 128
#endif
#ifndef VRT_ORD_DIV
#define VRT_ORD_DIV 4
#endif
#ifndef VRT_ORD_MIN_ROUNDS
#define VRT_ORD_MIN_ROUNDS 1
#endif
#ifndef VRT_DEFER_GRID_DIV
#define VRT_DEFER_GRID_DIV 8
#endif
#ifndef VRT_DEFER_GRID_DIV_COLOR
#define VRT_DEFER_GRID_DIV_COLOR VRT_DEFER_GRID_DIV
#endif
#ifndef VRT_QUERY_WG_WAVES
#define VRT_QUERY_WG_WAVES 1
#endif
#ifndef VRT_TRACE_WG_WAVES
#define VRT_TRACE_WG_WAVES 1
#endif
#ifndef VRT_TRACE_MIN_WAVES
#define VRT_TRACE_MIN_WAVES 6
#endif
#ifndef VRT_SPATIAL_LDS_STEPS
#define VRT_SPATIAL_LDS_STEPS 0x16
#endif

namespace vrt {

// Waves per workgroup, each rendering an 8x8 pixel tile. Two (a 16x8 tile): a finished
// workgroup frees its slots two waves at a time, so the dispatcher refills them sooner than with
// four-wave 16x16 workgroups (C3 -4.4 %, C2 -2.8 %, C4 -8.1 % per frame; one wave per workgroup:
// C3 -1.7 %, profiles/r02_s06). Images are identical at 1, 2 and 4.
constexpr int kWgWaves = VRT_WG_WAVES;
static_assert(kWgWaves == 1 || kWgWaves == 2 || kWgWaves == 4, "1, 2 or 4 waves per workgroup");

// Waves per SIMD the register budget is sized for: 7 -> 72 VGPRs. With certified walks inside the
// bounce stacks, 64 VGPRs (8 waves) spill in the glass waves that bound a frame: 7 is 2-4 % faster
// on C1-C4 (profiles/r01_v56_ab_occupancy.log), 6 (80 VGPRs) no better.
constexpr int kMinWaves = VRT_MIN_WAVES;
// The certified pass without the exact path (render_kernel's DEFER instances) fits 64 VGPRs (8
// waves per SIMD) with 8 bytes of scratch, but runs faster at 7 (72 VGPRs, no spills): C3 0.0464 ->
// 0.0447, C4 0.1751 -> 0.1605, textured C3 -4 % (profiles/r03_s11, r03_s12); 6 is slower again.
// Re-tested at 65 VGPRs (r08, the factored bound): at 8 waves the DEFER instances still need 2
// spilled VGPRs, 8 bytes of scratch and 74-140 SGPR spills against 16-58, and run slower,
// alternating with the 7-wave library, ms per frame 7 -> 8: C3 0.0346 / 0.0346 / 0.0348 -> 0.0358 /
// 0.0362 / 0.0358, C2 0.0530 / 0.0529 -> 0.0550 / 0.0548, C4 0.1210 / 0.1209 -> 0.1300 / 0.1305, C1
// 0.1207 / 0.1205 -> 0.1204 / 0.1205 (profiles/r08_walk/ab_bench.txt). 7 stays: as the floor the
// instances are built for. Since r09 (cert_walk's result no longer carried through its loop) the
// DEFER instances without trees take 56 VGPRs, spill nothing and run 8 to a SIMD, which is now the
// faster state: capped at 7 by kDeferLdsPad below, C3 0.0332 / 0.0334 / 0.0333 -> 0.0344 / 0.0345 /
// 0.0343 ms per frame (profiles/r09_exit/ab_occupancy.txt).
constexpr int kDeferWaves = VRT_DEFER_WAVES;
// Dynamic LDS bytes per workgroup of the certified pass without trees (launch_render): an occupancy
// cap for A/B builds. kDeferWaves is a floor: since the one-exit walk loop (r09) the DEFER instances
// take 56 VGPRs and the hardware runs them 8 waves to a SIMD. 11264 bytes let 14 two-wave workgroups
// share a CU's 160 KiB: 7 waves per SIMD.
constexpr uint32_t kDeferLdsPad = VRT_DEFER_LDS_PAD;
// resident waves per SIMD of the exact pass's whole-frame instance (see exact_pass_kernel, WAVES)
constexpr int kExactWaves = VRT_EXACT_WAVES;
// VGPR cap of the exact pass's colour whole-frame instances (exact_pass_kernel_capped): a budget between
// the whole-wave steps kExactWaves can express (72, 80, 96, 128). 0: no cap, the instance is the kExactWaves
// one. A capped instance promises 512 / cap waves per SIMD (the cap in 8-register granules) and carries
// amdgpu_num_vgpr, which the compiler honours inside that promise (exact_cap_attr below).
// 120: the smallest budget at which both instances spill no VGPR and their scratch is the bounce stack's
// 544 B per lane (112: one spilled VGPR in the one-frame instance; 104: 4 and 7; 96: 10 and 12). A SIMD
// full of certified waves holds 8 x 56 of its 512 VGPRs: the 72-VGPR exact wave already needed one of them
// to leave, and with one gone 120 are free, so the wider wave displaces no more certified waves than the
// narrow one did. C3 ms per frame, make variant builds and the parent alternating, three runs each
// (profiles/r13_exact/screen.txt): parent 0.0303-0.0304; the restructured source at 72 VGPRs
// 0.0294-0.0295; 96: 0.0290-0.0294; 112: 0.0288-0.0289; 120: 0.0286-0.0287; 128: 0.0287-0.0288; 160 (3
// waves): 0.0286 / 0.0288 / 0.0306; a lone frame 0.1014-0.1036 -> 0.0885-0.0900 ms at 120. The product
// library against the parent, alternating (profiles/r13_exact/ab_bench.txt): C3 0.0305 x 4 -> 0.0286-0.0288,
// C1 0.1086-0.1088 -> 0.1068-0.1070, C2 0.0471-0.0474 -> 0.0466-0.0467, C4 0.1054 -> 0.1052-0.1057.
// Textured whole frames keep the kExactWaves instance: under a cap of 120 it compiles to 1 spilled VGPR and
// 560 B of scratch, under 96 to 33-35 spilled, and neither has been timed.
constexpr int kExactVgprs = VRT_EXACT_VGPRS;
static_assert(kExactVgprs == 0 || (kExactVgprs >= 64 && kExactVgprs <= 256 && kExactVgprs % 8 == 0),
              "a VGPR cap of 64 to 256 in whole allocation granules, or 0 for none");
// waves per SIMD a cap of v VGPRs allows (allocation granule: 8 registers of the SIMD's 512)
constexpr int exact_cap_waves(int v) { return v > 0 ? 512 / ((v + 7) / 8 * 8) : 1; }
// the attribute's argument for a cap of v registers: gfx90a and later share one file between VGPRs and
// AGPRs, and the compiler takes the argument as half of it (it doubles the number; a value above the
// promised waves' own budget it drops without a word: make asm shows the registers an instance got)
constexpr int exact_cap_attr(int v) { return v > 0 ? v / 2 : 256; }
// resident waves per SIMD of the certified pass with certified trees
constexpr int kTreeWaves = VRT_TREE_WAVES;
// resident waves per SIMD of the exact pass's short-band instance (see exact_pass_kernel, WAVES)
constexpr int kFatWaves = VRT_FAT_WAVES;

// pixels per sparse batch of the exact pass (<= 64): a sparse wave lasts as long as its slowest
// walk and its steps execute the union of its lanes' sampled steps, so smaller batches shorten the
// exact pass's span, which the frame's latency and a short run's drain wait for, at more waves: 32
// with the column-block segments: the driver's 20-frame C3 command 0.0500 -> 0.0464 ms, latency
// 0.123 -> 0.106 ms, 500 frames +0.8 % (C4 +-0, C2 +1 %); 16: 0.0485 / 0.103 / +2.6 %; 8: 0.0479 /
// 0.102 / +6 % (profiles/r05_s10). Measured again on the 120-VGPR instance (r13, kExactVgprs): 16 against
// 32, three alternating runs, C3 0.0293-0.0294 against 0.0286-0.0287 ms per frame (+2.3 %), a lone frame
// 0.0796-0.0813 against 0.0885-0.0900 ms, the 20-frame command 0.0345-0.0349 against 0.0348-0.0358: 32 stays
// (profiles/r13_exact/screen.txt)
constexpr uint32_t kSparseBatch = VRT_SPARSE_BATCH;
// the same for textured frames: 64 (many more sparse pixels, texel-edge hits: at 32 the extra waves
// cost textured C3 0.0572 -> 0.0661 ms, C4 0.2329 -> 0.2894; profiles/r05_s30)
constexpr uint32_t kSparseBatchTex = VRT_SPARSE_BATCH_TEX;
// the same in the exact pass's short-band instance (see exact_pass_kernel, SB)
constexpr uint32_t kSparseBatchFat = VRT_SPARSE_BATCH_FAT;
// wave priority of the whole exact pass (0: only its bounce stacks raise it): its few long waves
// share SIMDs with the next frames' certified waves; at 2 their chains issue first (C3 0.0395 ->
// 0.0387 ms per frame, C4 -1 %, the driver's 20-frame run 0.0531 -> 0.0509; 3: C3 0.0389,
// profiles/r04_exact/)
constexpr int kExactPrio = VRT_EXACT_PRIO;

// cap of the octant forward distance F (G = F - 1 in 8 bits): 128 vs 64 C4 -1.4 %, C1-C3 +-0.3 % (r03_s42)
constexpr uint32_t kFwdCap = VRT_FWD_CAP;
static_assert(kFwdCap >= 3 && kFwdCap <= 255, "F and G are stored in 8 bits");

// first-pass slots per class of a tile-order launch: tiles / (8 kOrdDiv), i.e. up to a quarter of
// the tiles in the heavy-first pass (C3: ~1600 of a part launch's 8160 tiles are heavy); ord_q_for
constexpr uint32_t kOrdDiv = VRT_ORD_DIV;
// dispatch rounds of waves from which an in-lane launch takes the tile order
constexpr uint32_t kOrdMinRounds = VRT_ORD_MIN_ROUNDS;
// certified-pass waves per exact-pass workgroup (the exact pass's grid; a workgroup loops over the
// batches beyond it): 8 covers textured frames' deferred pixels in one batch per workgroup (textured
// C3 0.0843 -> 0.0713 ms against 32; 4 no better; profiles/r03_s11, r03_s12)
constexpr uint32_t kDeferGridDiv = VRT_DEFER_GRID_DIV;
constexpr uint32_t kDeferGridDivColor = VRT_DEFER_GRID_DIV_COLOR;  // the same for colour-only frames

// waves per workgroup of the ray-query kernel (vrt_query_kernels.h). One: a wave lasts as long as its
// longest ray and shares nothing with its neighbours (no barrier, a 3 KB axis table of its own), so a
// one-wave workgroup returns its slot the moment that ray ends, as in the exact pass. No larger value
// has been measured.
constexpr int kQueryWgWaves = VRT_QUERY_WG_WAVES;
static_assert(kQueryWgWaves >= 1 && kQueryWgWaves <= 4, "1 to 4 waves per query workgroup");
// the same for the shaded ray-query kernel (vrt_trace_kernels.h), where the reasoning holds more strongly:
// a wave lasts as long as its longest bounce tree. Its LDS (the axis table and the bounce stack's bottom
// entry: 5.25 KB per wave) does not bound occupancy at one wave. Two: the coherent arms within 1.4 % either
// way, scattered rays 1.4-2.1 % slower (profiles/ray_trace_ab.txt).
constexpr int kTraceWgWaves = VRT_TRACE_WG_WAVES;
static_assert(kTraceWgWaves >= 1 && kTraceWgWaves <= 4, "1 to 4 waves per trace workgroup");
// resident waves per SIMD the shaded ray-query kernel is built for. Without a promise (1) the four
// instances take 87-93 VGPRs: 5 waves, no spills. 6 -> 80 VGPRs with at most one spilled VGPR, and every
// pixel of the 1920x1080 benchmark camera in tile order 0.2578 -> 0.2478 ms at C3, 0.3896 -> 0.3673 at C1,
// 2 M scattered rays 5.90 -> 5.47 and 5.75 -> 5.36 ms; 7 (72 VGPRs, 1-21 spilled) is no faster: 0.2505,
// 0.3678, 5.45, 5.32 (profiles/ray_trace_ab.txt; the frame's STATS instance runs at 7 with 24-40 spilled)
constexpr int kTraceMinWaves = VRT_TRACE_MIN_WAVES;

// the steps at which a spatial-filter pass (vrt_spatial_kernels.h) launches its LDS-staged form, bit `step` for
// step 1, 2 and 4 (the steps that have one); every other step, and a cleared bit, launch the direct gather.
// 0x16: staged at all three. One pass over 1920x1080 at C3, FACE guide, no count buffer, the product library
// against a VRT_SPATIAL_LDS_STEPS=0 build (each three runs of 21 launches in a process of its own, ms staged ->
// direct): step 1 0.0246 -> 0.0482, step 2 0.0259 -> 0.0479, step 4 0.0294 -> 0.0472; the direct gather at step 8
// 0.0468 and 0.0469 in the two processes, at step 16 0.0528 and 0.0527 (profiles/spatial_bench.txt)
constexpr uint32_t kSpatialLdsSteps = VRT_SPATIAL_LDS_STEPS;
static_assert((kSpatialLdsSteps & ~0x16u) == 0, "only steps 1, 2 and 4 have an LDS-staged form");

// The once-per-pixel cuts of the certified pass's DEFER instances (r16), each switched off by a
// define of its own in a diagnostic build (make variant NAME=nosky DEFS=-DVRT_NO_SKY_ZERO), for the per-cut
// counter table (profiles/r16_ndc_sky/flag_cuts.txt). Images are identical with either of them off.
//  - kCutSky: a primary miss's sun disc without log and exp where no missing lane of the wave is near the sun;
//  - kCutSpec: the specular power of a colour-only primary hit by the bare v_log_f32 / v_exp_f32.
#ifdef VRT_NO_SKY_ZERO
constexpr bool kCutSky = false;
#else
constexpr bool kCutSky = true;
#endif
#ifdef VRT_NO_RAW_SPECULAR
constexpr bool kCutSpec = false;
#else
constexpr bool kCutSpec = true;
#endif

}  // namespace vrt

#endif  // VRT_TUNING_H
