// vrt_filters.cpp — the post-filters on a frame and the ID pass's buffers, all on the first device: the reprojected
// temporal filter, the ID-guided spatial filter, the loop that runs both (vrt_render_frame_reprojected) and its
// setters (vrt_context.h). The ID pass itself is vrt_queries.cpp.
#include <cstring>

#include "vrt_context.h"

using namespace vrt;

extern "C" {

// ---- reprojected temporal filter (vrt_reproject_kernels.h) --------------------------------------

// What vrt_reproject_temporal_async checks beyond check_ids (which takes the band's ids and depth)
static int check_reproject(vrt_ctx* ctx, const vrt_camera* cam, const float* prev_pv, int32_t prev_pitch,
                           const void* raw, const void* depth, const void* prev, const void* prev_ids, const void* out,
                           const void* src) {
  if (!prev_pv) return fail(ctx, VRT_ERR_INVALID, "null previous matrix");
  if (!raw || !depth || !out) return fail(ctx, VRT_ERR_INVALID, "null raw, depth or output buffer");
  if (prev_pitch < cam->width) return fail(ctx, VRT_ERR_INVALID, "previous row pitch must be >= the image width");
  if ((prev == nullptr) != (prev_ids == nullptr))
    return fail(ctx, VRT_ERR_INVALID, "the previous frame and its id buffer are given together or not at all");
  if (prev && out == prev) return fail(ctx, VRT_ERR_INVALID, "the output must not alias the previous frame");
  const uintptr_t words = reinterpret_cast<uintptr_t>(raw) | reinterpret_cast<uintptr_t>(prev) |
                          reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(src);
  if ((words & 3u) != 0 || (reinterpret_cast<uintptr_t>(prev_ids) & 7u) != 0)
    return fail(ctx, VRT_ERR_INVALID, "device id buffers must be 8-byte aligned, the other buffers 4-byte aligned");
  return VRT_OK;
}

// One reprojection launch over rows [row0, row0 + rows) (rows >= 1) on `st`: no allocation, no host
// synchronisation. eb / ee: the launch's device timestamps (optional). fetch, d_taps: the fetch mode and the
// optional tap masks of vrt_reproject_temporal_fetch_async
static int enqueue_reproject(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, const float* prev_pv, float alpha,
                             int32_t row0, int32_t rows, int32_t pitch, const uint32_t* d_raw, const vrt_pixel_id* d_ids,
                             const float* d_depth, const uint32_t* d_prev, const vrt_pixel_id* d_prev_ids,
                             int32_t prev_pitch, uint32_t* d_out, int32_t* d_src, hipStream_t st, hipEvent_t eb,
                             hipEvent_t ee, int32_t fetch, uint8_t* d_taps) {
  Shard& s = ctx->sh[0];
  // the frame's argument block, as enqueue_ids fills it: primary_ray reads it
  vrt::KArgs a = make_args(ctx, s, cam, p, row0, rows, 1);
  a.pitch = pitch;
  vrt::ReprojArgs r;
  std::memcpy(r.pv, prev_pv, sizeof(r.pv));
  r.alpha = alpha;
  r.prev_pitch = prev_pitch;
  r.raw = d_raw;
  r.ids = reinterpret_cast<const uint2*>(d_ids);
  r.depth = d_depth;
  r.prev = d_prev;
  r.prev_ids = reinterpret_cast<const uint2*>(d_prev_ids);
  r.out = d_out;
  r.src = d_src;
  vrt::launch_reproject(a, r, fetch, d_taps, st, eb, ee);
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

int vrt_reproject_temporal_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, const float prev_pv[16],
                                 float alpha, int32_t row0, int32_t rows, int32_t pitch, const uint32_t* d_raw_rgba8,
                                 const vrt_pixel_id* d_ids, const float* d_depth, const uint32_t* d_prev_rgba8,
                                 const vrt_pixel_id* d_prev_ids, int32_t prev_pitch, uint32_t* d_out_rgba8,
                                 int32_t* d_src, void* hip_stream) {
  // the nearest fetch without tap masks: the same checks in the same order, the same launch
  return vrt_reproject_temporal_fetch_async(ctx, cam, p, prev_pv, alpha, VRT_FETCH_NEAREST, row0, rows, pitch,
                                            d_raw_rgba8, d_ids, d_depth, d_prev_rgba8, d_prev_ids, prev_pitch,
                                            d_out_rgba8, d_src, nullptr, hip_stream);
}

int vrt_reproject_temporal_fetch_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, const float prev_pv[16],
                                       float alpha, int32_t fetch, int32_t row0, int32_t rows, int32_t pitch,
                                       const uint32_t* d_raw_rgba8, const vrt_pixel_id* d_ids, const float* d_depth,
                                       const uint32_t* d_prev_rgba8, const vrt_pixel_id* d_prev_ids, int32_t prev_pitch,
                                       uint32_t* d_out_rgba8, int32_t* d_src, uint8_t* d_taps, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_ids(ctx, cam, p, row0, rows, pitch, d_ids, d_depth, true);
  if (st != VRT_OK) return st;
  st = check_reproject(ctx, cam, prev_pv, prev_pitch, d_raw_rgba8, d_depth, d_prev_rgba8, d_prev_ids, d_out_rgba8,
                       d_src);
  if (st != VRT_OK) return st;
  if (fetch != VRT_FETCH_NEAREST && fetch != VRT_FETCH_BILINEAR) return fail(ctx, VRT_ERR_INVALID, "unknown fetch mode");
  if (rows == 0) return VRT_OK;
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  return enqueue_reproject(ctx, cam, p, prev_pv, alpha, row0, rows, pitch, d_raw_rgba8, d_ids, d_depth, d_prev_rgba8,
                           d_prev_ids, prev_pitch, d_out_rgba8, d_src, static_cast<hipStream_t>(hip_stream), eb, ee,
                           fetch, d_taps);
}

// ---- ID-guided spatial filter (vrt_spatial_kernels.h) -------------------------------------------

// What a pass's guide and range may be
static int check_spatial_guide(vrt_ctx* ctx, int32_t guide, int32_t range) {
  if (guide != VRT_GUIDE_FACE && guide != VRT_GUIDE_PLANE) return fail(ctx, VRT_ERR_INVALID, "unknown guide");
  if (range < 0) return fail(ctx, VRT_ERR_INVALID, "range must be >= 0");
  return VRT_OK;
}

// One pass over rows [row0, row0 + rows) (rows >= 1) on `st`: one launch, no allocation, no host
// synchronisation. eb / ee: the launch's device timestamps (optional)
static int enqueue_spatial(vrt_ctx* ctx, int32_t w, int32_t h, int32_t pitch, int32_t step, int32_t guide, int32_t range,
                           int32_t row0, int32_t rows, const uint32_t* d_in, const vrt_pixel_id* d_ids,
                           const uint8_t* d_keep, uint32_t* d_out, uint8_t* d_count, hipStream_t st, hipEvent_t eb,
                           hipEvent_t ee) {
  vrt::SpatialArgs a;
  a.width = w;
  a.height = h;
  a.pitch = pitch;
  a.step = step;
  a.guide = guide;
  a.range = range;
  a.row0 = row0;
  a.rows = rows;
  a.nlog = uint32_t(__builtin_ctz(uint32_t(ctx->sh[0].n)));  // the edge is a power of two (vrt_upload_volume)
  a.in = d_in;
  a.ids = reinterpret_cast<const uint2*>(d_ids);
  a.keep = d_keep;
  a.out = d_out;
  a.count = d_count;
  vrt::launch_spatial(a, st, eb, ee);
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

int vrt_spatial_filter_async(vrt_ctx* ctx, int32_t width, int32_t height, int32_t pitch, int32_t step, int32_t guide,
                             int32_t range, int32_t row0, int32_t rows, const uint32_t* d_in_rgba8,
                             const vrt_pixel_id* d_ids, const uint8_t* d_keep, uint32_t* d_out_rgba8, uint8_t* d_count,
                             void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!ctx->sh[0].d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (!d_in_rgba8 || !d_ids || !d_out_rgba8) return fail(ctx, VRT_ERR_INVALID, "null input, id or output buffer");
  if (const int st = check_image(ctx, width, height); st != VRT_OK) return st;
  if (const int st = check_band(ctx, width, height, row0, rows, pitch, true); st != VRT_OK) return st;
  if (step < 1 || step > 64) return fail(ctx, VRT_ERR_INVALID, "step must be in [1, 64]");
  if (const int st = check_spatial_guide(ctx, guide, range); st != VRT_OK) return st;
  if (d_out_rgba8 == d_in_rgba8) return fail(ctx, VRT_ERR_INVALID, "the output must not alias the input");
  if ((reinterpret_cast<uintptr_t>(d_ids) & 7u) != 0 ||
      ((reinterpret_cast<uintptr_t>(d_in_rgba8) | reinterpret_cast<uintptr_t>(d_out_rgba8)) & 3u) != 0)
    return fail(ctx, VRT_ERR_INVALID, "device id buffer must be 8-byte aligned, the colour buffers 4-byte aligned");
  if (rows == 0) return VRT_OK;
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  return enqueue_spatial(ctx, width, height, pitch, step, guide, range, row0, rows, d_in_rgba8, d_ids, d_keep,
                         d_out_rgba8, d_count, static_cast<hipStream_t>(hip_stream), eb, ee);
}

int vrt_spatial_filter(vrt_ctx* ctx, int32_t width, int32_t height, int32_t passes, int32_t guide, int32_t range,
                       const uint8_t* rgba8, const vrt_pixel_id* ids, const uint8_t* keep, uint8_t* out_rgba8) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!ctx->sh[0].d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (!rgba8 || !ids || !out_rgba8) return fail(ctx, VRT_ERR_INVALID, "null input, id or output buffer");
  int st = check_image(ctx, width, height);
  if (st != VRT_OK) return st;
  if (passes < 1 || passes > 5) return fail(ctx, VRT_ERR_INVALID, "passes must be in [1, 5]");
  if ((st = check_spatial_guide(ctx, guide, range)) != VRT_OK) return st;
  DeviceGuard guard;
  Shard& s = ctx->sh[0];
  VRT_HIP(ctx, hipSetDevice(s.device));
  const size_t px = size_t(width) * size_t(height);
  // the staging: synchronous calls only, so no launch still uses buffers that are replaced here
  if (ctx->d_sp_ids.cap < px && !stage_alloc_all(px, ctx->d_sp_rgba[0], ctx->d_sp_rgba[1], ctx->d_sp_ids, ctx->d_sp_keep))
    return fail(ctx, VRT_ERR_OOM, "hipMalloc spatial-filter staging");
  hipStream_t qs = main_stream(s);
  VRT_HIP(ctx, hipMemcpyAsync(ctx->d_sp_rgba[0].p, rgba8, px * 4, hipMemcpyHostToDevice, qs));
  VRT_HIP(ctx, hipMemcpyAsync(ctx->d_sp_ids.p, ids, px * sizeof(vrt_pixel_id), hipMemcpyHostToDevice, qs));
  if (keep) VRT_HIP(ctx, hipMemcpyAsync(ctx->d_sp_keep.p, keep, px, hipMemcpyHostToDevice, qs));
  for (int32_t q = 0; q < passes; ++q) {  // pass q at step 2^q, from frame q & 1 into the other
    hipEvent_t eb, ee;
    launch_timing_events(ctx, eb, ee);
    st = enqueue_spatial(ctx, width, height, width, 1 << q, guide, range, 0, height, ctx->d_sp_rgba[q & 1].p,
                         ctx->d_sp_ids.p, keep ? ctx->d_sp_keep.p : nullptr, ctx->d_sp_rgba[(q & 1) ^ 1].p, nullptr, qs,
                         eb, ee);
    if (st != VRT_OK) return st;
  }
  VRT_HIP(ctx, hipMemcpyAsync(out_rgba8, ctx->d_sp_rgba[passes & 1].p, px * 4, hipMemcpyDeviceToHost, qs));
  VRT_HIP(ctx, hipStreamSynchronize(qs));
  return VRT_OK;
}

int vrt_set_reprojected_spatial(vrt_ctx* ctx, int32_t mode, int32_t passes, int32_t guide, int32_t range) {
  if (!ctx) return VRT_ERR_INVALID;
  if (mode != VRT_SPATIAL_OFF && mode != VRT_SPATIAL_DISPLAY && mode != VRT_SPATIAL_FILL)
    return fail(ctx, VRT_ERR_INVALID, "unknown spatial mode");
  if (passes < 1 || passes > 5) return fail(ctx, VRT_ERR_INVALID, "passes must be in [1, 5]");
  if (const int st = check_spatial_guide(ctx, guide, range); st != VRT_OK) return st;
  // the history (frames, IDs, matrix) stays: only the next calls' passes change
  ctx->rp_spatial = mode;
  ctx->rp_sp_passes = passes;
  ctx->rp_sp_guide = guide;
  ctx->rp_sp_range = range;
  return VRT_OK;
}

// The staging of vrt_render_frame_reprojected on the first device (the current one), for frames of w x h:
// the raw frame, the depth, and ping-pong filtered frames and ID buffers. Synchronous calls only, so no
// launch still uses buffers that are replaced here. A new size drops the history.
static int ensure_reproject_stage(vrt_ctx* ctx, int32_t w, int32_t h) {
  if (w == ctx->rp_w && h == ctx->rp_h) return VRT_OK;
  const size_t px = size_t(w) * size_t(h);
  ctx->rp_w = ctx->rp_h = 0;
  ctx->rp_valid = false;
  if (ctx->d_rp_raw.cap < px && !stage_alloc_all(px, ctx->d_rp_raw, ctx->d_rp_depth, ctx->d_rp_out[0], ctx->d_rp_out[1],
                                                 ctx->d_rp_ids[0], ctx->d_rp_ids[1]))
    return fail(ctx, VRT_ERR_OOM, "hipMalloc reprojected-frame staging");
  if (!ctx->ev_rp_beg) VRT_HIP(ctx, hipEventCreate(&ctx->ev_rp_beg));
  if (!ctx->ev_rp_end) VRT_HIP(ctx, hipEventCreate(&ctx->ev_rp_end));
  ctx->rp_w = w;
  ctx->rp_h = h;
  return VRT_OK;
}

int vrt_render_frame_reprojected(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, float alpha,
                                 uint8_t* out_rgba8, vrt_stats* stats) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_render_args(ctx, cam, p);
  if (st != VRT_OK) return st;
  if (!out_rgba8) return fail(ctx, VRT_ERR_INVALID, "null output");
  if (stats && (stats->request & VRT_STATS_COUNTERS))
    return fail(ctx, VRT_ERR_UNSUPPORTED, "vrt_render_frame_reprojected does not count");
  DeviceGuard guard;
  Shard& s = ctx->sh[0];
  VRT_HIP(ctx, hipSetDevice(s.device));
  const int32_t w = cam->width, h = cam->height;
  if ((st = ensure_reproject_stage(ctx, w, h)) != VRT_OK) return st;
  const size_t bytes = size_t(w) * size_t(h) * 4;
  if ((st = ensure_stage(ctx, bytes)) != VRT_OK) return st;
  // the spatial passes' staging, with the first frame that runs them (the history is not touched)
  const int32_t spatial = ctx->rp_spatial, passes = ctx->rp_sp_passes;
  if (spatial != VRT_SPATIAL_OFF && ctx->d_rp_taps.cap < size_t(w) * size_t(h) &&
      !stage_alloc_all(size_t(w) * size_t(h), ctx->d_rp_sp[0], ctx->d_rp_sp[1], ctx->d_rp_taps))
    return fail(ctx, VRT_ERR_OOM, "hipMalloc reprojected-frame spatial staging");
  hipStream_t ms = main_stream(s);
  const int cur = ctx->rp_cur ^ 1, prev = ctx->rp_cur;
  // 1. the quantised ray-traced frame: the temporal band path at u_Alpha = 1 (its output is the raw frame)
  vrt::KArgs a = make_args(ctx, s, cam, p, 0, h, 1);
  a.alpha = 1.0f;
  a.prev = ctx->d_rp_raw.p;
  a.cur = ctx->d_rp_raw.p;
  launch(ctx, s, a, nullptr, nullptr, nullptr, ms, stats ? ctx->ev_rp_beg : nullptr, nullptr);
  VRT_HIP(ctx, hipGetLastError());
  // 2. noise-free geometry buffers: a noised primary ray's hit belongs at another screen position
  vrt_params geom = *p;
  geom.ray_noise = 0.0f;
  if ((st = enqueue_ids(ctx, cam, &geom, 0, h, w, ctx->d_rp_ids[cur].p, ctx->d_rp_depth.p, ms)) != VRT_OK) return st;
  // 3. the filter against the previous call's frame, IDs and matrix
  // (VRT_SPATIAL_FILL: into a staging frame, with the tap bytes the passes keep pixels by; the passes end in the
  // history frame)
  const bool hist = ctx->rp_valid, fill = spatial == VRT_SPATIAL_FILL;
  hipEvent_t ev_end = stats ? ctx->ev_rp_end : nullptr;
  uint32_t* filtered = fill ? ctx->d_rp_sp[0].p : ctx->d_rp_out[cur].p;
  st = enqueue_reproject(ctx, cam, &geom, ctx->rp_pv, alpha, 0, h, w, ctx->d_rp_raw.p, ctx->d_rp_ids[cur].p, ctx->d_rp_depth.p,
                         hist ? ctx->d_rp_out[prev].p : nullptr, hist ? ctx->d_rp_ids[prev].p : nullptr, w, filtered,
                         nullptr, ms, nullptr, spatial == VRT_SPATIAL_OFF ? ev_end : nullptr, ctx->rp_fetch,
                         fill ? ctx->d_rp_taps.p : nullptr);
  if (st != VRT_OK) return st;
  // 3b. the spatial passes on this frame's noise-free IDs, pass q at step 2^q. DISPLAY: from the history frame
  // through the staging frames, the history stays unfiltered. FILL: from staging frame 0, alternating, the last
  // pass into the history frame
  const uint32_t* shown = filtered;
  if (spatial != VRT_SPATIAL_OFF) {
    for (int32_t q = 0; q < passes; ++q) {
      const bool last = q + 1 == passes;
      uint32_t* dst = fill ? (last ? ctx->d_rp_out[cur].p : ctx->d_rp_sp[(q + 1) & 1].p) : ctx->d_rp_sp[q & 1].p;
      st = enqueue_spatial(ctx, w, h, w, 1 << q, ctx->rp_sp_guide, ctx->rp_sp_range, 0, h, shown, ctx->d_rp_ids[cur].p,
                           fill ? ctx->d_rp_taps.p : nullptr, dst, nullptr, ms, nullptr, last ? ev_end : nullptr);
      if (st != VRT_OK) return st;
      shown = dst;
    }
  }
  // 4. to the host through the pinned staging
  VRT_HIP(ctx, hipMemcpyAsync(ctx->h_stage.p, shown, bytes, hipMemcpyDeviceToHost, ms));
  VRT_HIP(ctx, hipStreamSynchronize(ms));
  std::memcpy(out_rgba8, ctx->h_stage.p, bytes);
  if (stats) {  // the span from the first launch's start to the last launch's end, as vrt_render_frame's
    float ms_span = 0.0f;
    VRT_HIP(ctx, hipEventElapsedTime(&ms_span, ctx->ev_rp_beg, ctx->ev_rp_end));
    stats->kernel_ms = ms_span;
  }
  // this frame is the next call's history, if its camera has a forward matrix
  ctx->rp_cur = cur;
  ctx->rp_valid = vrt_camera_forward(cam, ctx->rp_pv) == VRT_OK;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_reprojected_history_reset(vrt_ctx* ctx) {
  if (!ctx) return VRT_ERR_INVALID;
  ctx->rp_valid = false;
  return VRT_OK;
}

int vrt_set_reprojected_fetch(vrt_ctx* ctx, int32_t fetch) {
  if (!ctx) return VRT_ERR_INVALID;
  if (fetch != VRT_FETCH_NEAREST && fetch != VRT_FETCH_BILINEAR)
    return fail(ctx, VRT_ERR_INVALID, "unknown fetch mode");
  ctx->rp_fetch = fetch;  // the history (frames, IDs, matrix) stays: only the next calls' filter changes
  return VRT_OK;
}

}  // extern "C"
