// vrt_internal.h — the interface between the kernels (vrt_render.hip and its headers) and the C-ABI context
// (vrt_context.h and the vrt_*.cpp files around it). Not installed; include/vrt.h is the public boundary.
#ifndef VRT_INTERNAL_H
#define VRT_INTERNAL_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "vrt.h"
#include "vrt_skipfield_plan.h"
#include "vrt_tuning.h"

namespace vrt {

// Per-launch kernel arguments (by value: one kernarg segment per launch).
struct KArgs {
  float inv_pv[16];
  float rcp_w, rcp_h;  // RN(1 / width), RN(1 / height) (host IEEE division): the NDC's divisions
  float sun[3];
  float sky_sy;      // max(u_SunDir.y, 0): the skybox's sun height factor (voxel.glsl:391), uniform
  float sun_n[3];    // normalize(u_SunDir), GLSL normalize semantics (host: same IEEE ops)
  float sun_rcp[3];  // RN(1 / sun_n): the shadow walk's per-axis reciprocals (uniform)
  float time, ray_noise, refl_noise, refr_noise, max_len;
  float fn;
  int32_t n, width, height;
  int32_t row0, rows, row_step;
  int32_t row_blk_sh;  // log2 of the band's row block (ABI v11): band row i -> frame row
                       // row0 + (i >> row_blk_sh) * row_step + (i & (2^row_blk_sh - 1))
  int32_t pitch; // pixels from one band row to the next in every output/history buffer (>= width)
  uint32_t ostride;  // bytes from one direction octant's packed volume to the next (0: one volume)
  int32_t max_refl, max_transp;
  // textured mode (!_COLOR_ONLY): atlas of atlas_size^2 RGBA8 words, row 0 = bottom
  int32_t textured, atlas_size, atlas_tex_size;
  const uint32_t* atlas;
  // temporal epilogue (cur != nullptr): RGB8 store + temporal.glsl blend instead of float RGBA
  float alpha;
  // the vertex stage's division operands are in range for every pixel and frame of the launch
  // (vertex_div_ranges_ok, vrt_launch_consts.cpp; primary_ray's div3_lean). In the padding before `prev`:
  // the layout is unchanged.
  uint32_t vdiv_ok;
  const uint32_t* prev;  // last filtered frame (RGBA8 words), band-local like the output
  uint32_t* cur;         // filtered frame written here
  uint32_t* raw;         // optional: the quantised ray-trace frame (the reference's rayTrace FBO)
  // stats-free colour-only launches (vrt_set_certified): 0 exact walks only, 1 certified walks
  // for the exact path's shadow and air-medium secondary rays, 2 also whole pixels first
  int32_t cert;
  // certified bounce trees (vrt_set_cert_trees, ABI v15): colour-only certified launches settle a
  // glass primary hit's whole bounce tree by certified walks (cert_tree) where they can
  int32_t tree;
  // tile dispatch order (stats-free launches, vrt_set_tile_order): nullptr = dispatch order, else
  // the band's order buffer: three sets of kOrdClasses list counters, the per-tile wave counters,
  // two rank sets of `tiles` words and two list sets of tiles + 8 words (see ordered_tile).
  // tiles_x: tiles per row; tiles: tiles of the launch; ord_r / ord_w: the rank and list set read /
  // written; ctr_r / ctr_w / ctr_z: the counter set read / appended to / zeroed; ord_q: first-pass
  // slots per class (grid = 8 * ord_q + tiles)
  uint32_t* order;
  uint32_t tiles_x, tiles, ord_r, ord_w, ctr_r, ctr_w, ctr_z, ord_q;
  // deferred exact pass (stats-free certified launches, vrt_set_exact_pass): nullptr = the exact
  // path runs in the certified pixel's own lane; else the certified pass appends the pixels that
  // need the exact path to a list (one atomic per wave with such pixels, on one of kOrdClasses
  // segment counters by workgroup % 8) and the exact pass renders them 64 to a wave. defer: the
  // launch slot's words (2 counter sets, then the list); defer_e: the counter set of this launch
  // (the exact pass zeroes the other one for the next launch on the stream); defer_seg: list
  // words per segment (a segment holds at most ceil(tiles / 8) tiles' pixels)
  uint32_t* defer;
  uint32_t defer_e, defer_seg;
  int32_t exact_fat;  // the exact pass's short-band instance (colour-only bands of < 4 rounds of waves, lone frames)
  // adaptive exact-pass grid: workgroups of this launch's exact pass (0: the tiles-based default)
  // and the slot's host-mapped word its workgroup 0 stores the batch count in
  uint32_t exact_grid;
  uint32_t* batches_out;
  // frame batches (vrt_render_temporal_batch_async, alpha 1): `nframes` frames of the same band in
  // one launch, frame f's tiles at [f * frame_tiles, (f + 1) * frame_tiles) of the grid (tiles =
  // nframes * frame_tiles); frame 0 is inv_pv / time / cur / raw above, frame f >= 1 is fb[f - 1]
  int32_t nframes;
  uint32_t frame_tiles;
  struct FrameB {
    float inv_pv[16];
    float time;
    uint32_t* cur;
    uint32_t* raw;
  } fb[7];
  // The shadow walk's functions of the sun alone (sun_consts, filled where sun_n and sun_rcp are): the
  // certified pass reads them late, after its primary walk (late_sun, vrt_cert.h); no other kernel does.
  // sun_ok: fast_path_ok(sun_n); sun_neg[b]: 0 where sun_n[b] > 0, else the sign bit (x ^ sun_neg is
  // the walk's sign-folded x); sun_step[b]: sun_n[b] > 0 ? 1 : -1; sun_obase: the sun's octant volume,
  // ((x < 0) | (y < 0) << 1 | (z < 0) << 2) * ostride; sun_l1 = (|x| + |y|) + |z| and its products with
  // k24 = 2^-23 as cert_walk forms them: q2 = 0.5 k24 l1, b1 = k24 l1, g2 = 2 q2 (IEEE single, in that order)
  uint32_t sun_ok;
  uint32_t sun_neg[3];
  int32_t sun_step[3];
  uint32_t sun_obase;
  float sun_l1, sun_q2, sun_b1, sun_g2;
  // The certified pass's ray set-up and walk start (primary_ray<LEAN>, cert_pixel<LEAN>; no other kernel
  // reads them), read where first used and dead before the primary walk's loop.
  // Wave-uniform float work of the launch (setup_consts, filled where fn, width, height and max_len are;
  // IEEE single in the kernel's order): fw = float(width), fh = float(height), half_n = fn * 0.5,
  // walk_b0 = k24 (3 fn + 11) (cert_walk's b0), max_len2 = max_len + 2 (the primary walk's U + 2).
  float fw, fh, half_n, walk_b0, max_len2;
  // Per-launch proofs about the camera (cert_launch_consts, vrt_launch_consts.cpp; set by launch(), else 0):
  // kSetupW: n4.w = wn and f4.w = wf for every pixel, both Markstein-safe; rcp_wn, rcp_wf = RN(1 / w).
  // kSetupLen: every pixel's squared vdir length takes normalize3's rcp_newton(sqrt_fix(s)) with none
  // of its range tests. kSetupCell: every pixel's start P lies strictly inside the cell start_cell (in
  // [0, N)^3), away from its planes: start_fl1[b] = float(cell_b + 1) is floor(P_b) + 1 for a ray moving
  // up axis b, start_fl1[3 + b] = float(-cell_b) is floor(-P_b) + 1 for one moving down.
  uint32_t setup;
  float wn, wf, rcp_wn, rcp_wf;
  float start_fl1[6];
  int32_t start_cell[3];
};
constexpr uint32_t kSetupW = 1u, kSetupLen = 2u, kSetupCell = 4u;
// The launch proofs (host, vrt_launch_consts.cpp: arithmetic only, built without contraction):
// fills a.sun_n and a.sun_rcp from u_SunDir
void fill_sun(KArgs& a, const float* sun_dir);
// fills the sun_* constants above from a.sun_n and a.ostride
void sun_consts(KArgs& a);
// fills fw .. max_len2 above from a.width, a.height, a.fn and a.max_len
void setup_consts(KArgs& a);
// KArgs::vdiv_ok of one camera matrix
bool vertex_div_ranges_ok(const float* inv_pv);
// fills setup .. start_cell above from the launch's matrices, a.fn, a.n and a.vdiv_ok
void cert_launch_consts(KArgs& a);
constexpr int kMaxBatch = 8;  // frames per launch (1 + the fb entries)
constexpr int kWgThreads = 64 * kWgWaves;  // kWgWaves: vrt_tuning.h
constexpr int kTileW = kWgWaves >= 2 ? 16 : 8;  // a workgroup's pixel tile: 16x16, 16x8 or 8x8
constexpr int kTileH = kWgWaves == 4 ? 16 : 8;
constexpr int kMaxStack = 17;               // bounce-stack entries: max_reflections + max_transparencies + 1
constexpr int kCntReplicas = 256;           // counter replicas (per-wave atomics spread over them)
constexpr uint32_t kOrdClasses = 8;         // tile-order lists: tile % 8 (the XCD of its slot)
constexpr uint32_t kOrdCtrStride = 64;      // words between list counters (one 256-byte line each)
constexpr uint32_t kOrdHdr = 3 * kOrdClasses * kOrdCtrStride;  // tile-order buffer header: 3 counter sets
// first-pass slots per class of a tile-order launch (kOrdDiv, vrt_tuning.h)
__host__ __device__ inline uint32_t ord_q_for(uint32_t tiles) {
  return (tiles + kOrdClasses * kOrdDiv - 1u) / (kOrdClasses * kOrdDiv);
}
constexpr uint32_t kDeferHdr = 4 * kOrdClasses * kOrdCtrStride;  // deferred-pass slot header: 2 kinds x 2 sets
constexpr uint32_t kDeferDense = 32;        // deferred pixels from which a wave keeps its own exact-pass batch

// ---- launches (vrt_render.hip); all asynchronous on `s` ------------------------------------

// render_kernel, or for a deferred pair (a.defer on a stats-free a.cert 2 launch) the certified pass and then the
// exact pass over the pixels it left: the instances are rows of vrt_instances.h, chosen there (choose_instances)
// from stats, a.textured, a.cert, a.tree, a.order, a.defer, a.nframes and a.exact_fat. grid = a.tiles, or
// 8 * a.ord_q + a.tiles with a tile order (a.order); the pair's grids: at the launch. cnt_rep: the counter
// replicas (stats launches).
// ev_begin / ev_end (optional, timing events) are recorded when the kernel starts and ends on
// the device (hipExtLaunchKernelGGL), not when the host enqueues it; a pair records begin with its first
// kernel and end with its second.
void launch_render(const KArgs& a, bool stats, const uint16_t* vox, float4* out, vrt_hit* hit,
                   unsigned long long* cnt_rep, hipStream_t s, hipEvent_t ev_begin = nullptr,
                   hipEvent_t ev_end = nullptr);
// ray_query_kernel (vrt_query_kernels.h): `count` (>= 1) queries, one per lane, into hits. kind =
// VRT_CAST_NEAREST / VRT_CAST_OCCLUSION: `in` holds vrt_ray records and only a.n, a.fn and a.ostride are
// read; kQueryPick: `in` holds {px, py} pairs and `a` is the frame's argument block (make_args).
// ev_begin / ev_end: optional device timestamps, as launch_render's
constexpr int32_t kQueryPick = 2;
void launch_ray_query(const KArgs& a, int32_t kind, const uint16_t* vox, const void* in, uint32_t count,
                      vrt_ray_hit* hits, hipStream_t s, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// ray_trace_kernel (vrt_trace_kernels.h): `count` (>= 1) shaded queries, one per lane, into `out`; the
// instance is chosen from (kind, a.textured). `a` is a frame's argument block (make_args) with the caller's
// params. kTraceRays: `in` holds vrt_ray records, each with its own max_length (a.max_len, a.ray_noise and
// the camera fields are not read); kTracePixels: `in` holds {px, py} pairs of the frame `a` describes.
// ev_begin / ev_end: optional device timestamps, as launch_render's
constexpr int32_t kTraceRays = 0, kTracePixels = 1;
void launch_ray_trace(const KArgs& a, int32_t kind, const uint16_t* vox, const void* in, uint32_t count,
                      vrt_ray_color* out, hipStream_t s, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// cert_walks_debug_kernel (vrt_cert_debug_kernels.h; vrt_debug_cert_walks): `count` (>= 1) 32-byte ray records
// of `in`, one per lane, through the certified walk `kind` (0..3) into 32-byte result records; only a.n, a.fn
// and a.ostride are read. The volume must be the eight-octant layout (the certified walks' skip field).
void launch_cert_walks_debug(const KArgs& a, int32_t kind, const uint16_t* vox, const void* in, uint32_t count,
                             void* out, hipStream_t s);
// ids_exact_kernel (vrt_ids_kernels.h): rows [a.row0, a.row0 + a.rows) of the frame `a` describes (make_args
// with row_step 1; a.pitch pixels between rows of ids / depth; depth may be null), one launch, an 8x8 tile per
// one-wave workgroup. ev_begin / ev_end: optional device timestamps, as launch_render's. certified: the same
// grid of ids_cert_kernel instead (the volume must be the eight-octant layout, the certified walk's skip field):
// still one launch; n_exact (certified only, may be null): a device word the launch adds its exact-path pixels to
void launch_render_ids(const KArgs& a, const uint16_t* vox, vrt_pixel_id* ids, float* depth, hipStream_t s,
                       hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr, bool certified = false,
                       uint32_t* n_exact = nullptr);
// reproject_kernel and its two other fetch forms (vrt_reproject_kernels.h): the band `a` describes (make_args with row_step 1, as
// launch_render_ids; a.pitch pixels between band rows of raw, ids, depth, out and src), one launch, a 16x16
// tile per workgroup of kReprojWg threads. prev / prev_ids: the whole previous frame, prev_pitch pixels
// between rows, both null for "no history"; src may be null. ev_begin / ev_end: optional device timestamps
struct ReprojArgs {
  float pv[16];  // the previous frame's PV = inverse(inv_pv), column-major (vrt_camera_forward)
  float alpha;
  int32_t prev_pitch;
  const uint32_t* raw;
  const uint2* ids;
  const float* depth;
  const uint32_t* prev;
  const uint2* prev_ids;
  uint32_t* out;
  int32_t* src;
};
constexpr int kReprojWg = 256;
// fetch (one of the two modes: the caller checks) and taps, an optional tap-mask buffer (one byte per band pixel
// at a.pitch), choose the kernel: VRT_FETCH_NEAREST without taps reproject_kernel, with taps
// reproject_nearest_taps_kernel (the same pixels plus the byte); VRT_FETCH_BILINEAR reproject_bilinear_kernel
void launch_reproject(const KArgs& a, const ReprojArgs& r, int32_t fetch, uint8_t* taps, hipStream_t s,
                      hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// spatial_direct_kernel / spatial_lds_kernel (vrt_spatial_kernels.h): one à-trous pass over rows [row0, row0 +
// rows) of a width x height frame; every buffer whole-frame indexed, pixel (x, y) at [y * pitch + x]. keep and
// count may be null. nlog: log2 of the resident volume's edge (the PLANE guide's key). One launch, a 16x16 tile
// per workgroup of kSpatialWg threads; the form is chosen per step (kSpatialLdsSteps, vrt_tuning.h).
// ev_begin / ev_end: optional device timestamps
struct SpatialArgs {
  int32_t width, height, pitch, step, guide, range, row0, rows;
  uint32_t nlog;
  const uint32_t* in;
  const uint2* ids;
  const uint8_t* keep;
  uint32_t* out;
  uint8_t* count;
};
constexpr int kSpatialWg = 256;
// whether a pass at `step` launches the LDS-staged form
constexpr bool spatial_lds_form(int32_t step) {
  return (step == 1 || step == 2 || step == 4) && ((kSpatialLdsSteps >> step) & 1u) != 0;
}
void launch_spatial(const SpatialArgs& a, hipStream_t s, hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr);
// fold the counter replicas into dst (accumulating) and re-zero them
void launch_reduce_counters(unsigned long long* rep, unsigned long long* dst, hipStream_t s);
// in-place edit of the box [lo, lo + ext) (vrt_update_volume_region), inside [0, N)^3 (the texels it may change:
// volume_edit_plan, vrt_skipfield_plan.h):
// the box-local bytes `box` (device, x fastest) into the canonical volume; counts[0..4] (accumulating)
// = the box's glass and non-empty voxels before, the same after, cells whose emptiness changed
void launch_edit_apply(const uint8_t* box, uint8_t* vox, uint32_t n, const int32_t lo[3], const int32_t ext[3],
                       unsigned long long* counts, hipStream_t s);
// the kernel's packed volume(s) from the canonical N^3 bytes after a change inside the box [lo, lo + ext):
// 8 octant forward-distance volumes (octants == 8; tmp = 3 N^3 bytes) or one centred-distance volume
// (tmp = 2 N^3 bytes), rebuilt by the passes of skipfield_passes (vrt_skipfield_plan.h) in its order. An upload is the box [0, N)^3 (every
// texel, plane N included); distances = false (no cell's emptiness changed): the voxel bytes of the
// box only
void launch_volume_edit_passes(const uint8_t* vox, uint8_t* tmp, uint16_t* packed, uint32_t n, int octants,
                               const int32_t lo[3], const int32_t ext[3], bool distances, hipStream_t s);
// glass and non-empty voxel counts into out[0..1] (accumulating)
void launch_glass_share(const uint8_t* vox, uint64_t total, unsigned long long* out, hipStream_t s);
void launch_build_scene(uint8_t* vox, int scene, uint32_t n, const float* noise, hipStream_t s);
int run_fast_math_check(unsigned long long* host_out);  // vrt_debug_fast_math (7 counters)
int run_pow_forms_check(unsigned long long* host_out);  // vrt_debug_pow_forms (6 counters)
void launch_randomize(const float* dir, const float* pos, int n, float randomness, float seed,
                      float* out, hipStream_t s);
// frame rows [0, height) from k block-cyclic bands of 2^sh-row blocks, band_words words apart
// (band j's row i = frame row ((i >> sh) k + j) 2^sh + i % 2^sh), rows frame_pitch words apart
void launch_assemble_blocks(const uint32_t* bands, uint64_t band_words, int32_t k, int32_t sh, int32_t width,
                            int32_t height, uint32_t* frame, uint64_t frame_pitch, hipStream_t s);
// RGB8 wire format: RGBA8 words (A = 255) -> 3 bytes per pixel (pixels % 4 == 0, 16-byte aligned)
void launch_pack_rgb8(const uint32_t* rgba, uint64_t pixels, uint8_t* rgb, hipStream_t s);
// launch_assemble_blocks from RGB8 bands (band_px pixels apart), unpacked to RGBA8 words (width % 4 == 0)
void launch_assemble_blocks_rgb8(const uint8_t* bands, uint64_t band_px, int32_t k, int32_t sh, int32_t width,
                                 int32_t height, uint32_t* frame, uint64_t frame_pitch, hipStream_t s);

}  // namespace vrt

#endif  // VRT_INTERNAL_H
