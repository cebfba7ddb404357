// vrt_band_api.cpp — the asynchronous band entry points: one launch (or one batch of frames) of a caller's row
// band on the caller's stream, into the caller's buffers; no allocation, no host synchronisation (vrt_context.h).
#include <algorithm>
#include <cstring>

#include "vrt_context.h"

using namespace vrt;

extern "C" {

// Band arguments shared by the async entry points: rows inside the image, pitch >= width; blocks
// of row_block rows (a power of two <= 64) that do not overlap (row_step >= row_block unless the
// band is one block). *sh receives log2(row_block).
static int check_band(vrt_ctx* ctx, const vrt_camera* cam, int32_t row0, int32_t rows, int32_t row_step,
                      int64_t pitch, int32_t row_block = 1, int32_t* sh = nullptr) {
  int32_t b = 0;
  while (b < 7 && (1 << b) != row_block) ++b;
  if (b == 7) return fail(ctx, VRT_ERR_INVALID, "row_block must be a power of two in [1, 64]");
  if (sh) *sh = b;
  const int64_t last = rows > 0 ? int64_t(row0) + int64_t((rows - 1) >> b) * row_step + ((rows - 1) & (row_block - 1)) : 0;
  if (rows < 0 || row_step < 1 || row0 < 0 || (rows > row_block && row_step < row_block) ||
      (rows > 0 && last >= cam->height))
    return fail(ctx, VRT_ERR_INVALID, "row band outside the image");
  if (pitch < cam->width || pitch > INT32_MAX) return fail(ctx, VRT_ERR_INVALID, "row pitch must be >= the image width");
  return VRT_OK;
}

int vrt_render_blocks_pitched_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0,
                                    int32_t rows, int32_t row_step, int32_t row_block, int64_t pitch,
                                    float* d_out_rgba, vrt_hit* d_out_hit, uint64_t* d_counters, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_render_args(ctx, cam, p);
  if (st != VRT_OK) return st;
  if (!d_out_rgba) return fail(ctx, VRT_ERR_INVALID, "null output");
  int32_t sh = 0;
  if ((st = check_band(ctx, cam, row0, rows, row_step, pitch, row_block, &sh)) != VRT_OK) return st;
  if (rows == 0) return VRT_OK;
  Shard& s = ctx->sh[0];
  vrt::KArgs a = make_args(ctx, s, cam, p, row0, rows, row_step);
  a.row_blk_sh = sh;
  a.pitch = int32_t(pitch);
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  launch(ctx, s, a, reinterpret_cast<float4*>(d_out_rgba), d_out_hit,
         reinterpret_cast<unsigned long long*>(d_counters), static_cast<hipStream_t>(hip_stream), eb, ee);
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

int vrt_render_rows_pitched_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0,
                                  int32_t rows, int32_t row_step, int64_t pitch, float* d_out_rgba,
                                  vrt_hit* d_out_hit, uint64_t* d_counters, void* hip_stream) {
  return vrt_render_blocks_pitched_async(ctx, cam, p, row0, rows, row_step, 1, pitch, d_out_rgba, d_out_hit,
                                         d_counters, hip_stream);
}

int vrt_render_rows_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0, int32_t rows,
                          int32_t row_step, float* d_out_rgba, vrt_hit* d_out_hit, uint64_t* d_counters,
                          void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!cam) return fail(ctx, VRT_ERR_INVALID, "null camera");
  return vrt_render_rows_pitched_async(ctx, cam, p, row0, rows, row_step, cam->width, d_out_rgba, d_out_hit,
                                       d_counters, hip_stream);
}

int vrt_render_temporal_blocks_pitched_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p,
                                             float alpha, int32_t row0, int32_t rows, int32_t row_step,
                                             int32_t row_block, int64_t pitch, const uint32_t* d_prev_rgba8,
                                             uint32_t* d_cur_rgba8, uint32_t* d_raw_rgba8, vrt_hit* d_out_hit,
                                             uint64_t* d_counters, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_render_args(ctx, cam, p);
  if (st != VRT_OK) return st;
  if (!d_prev_rgba8 || !d_cur_rgba8) return fail(ctx, VRT_ERR_INVALID, "null history or output");
  int32_t sh = 0;
  if ((st = check_band(ctx, cam, row0, rows, row_step, pitch, row_block, &sh)) != VRT_OK) return st;
  if (rows == 0) return VRT_OK;
  Shard& s = ctx->sh[0];
  vrt::KArgs a = make_args(ctx, s, cam, p, row0, rows, row_step);
  a.row_blk_sh = sh;
  a.pitch = int32_t(pitch);
  a.alpha = alpha;
  a.prev = d_prev_rgba8;
  a.cur = d_cur_rgba8;
  a.raw = d_raw_rgba8;
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  launch(ctx, s, a, nullptr, d_out_hit, reinterpret_cast<unsigned long long*>(d_counters),
         static_cast<hipStream_t>(hip_stream), eb, ee);
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

// The per-launch fields of two frames' params agree (a frame batch's launch holds one copy of
// them; only the camera and u_Time are per frame)
static bool same_launch_params(const vrt_params& q, const vrt_params& r) {
  return q.sun_dir[0] == r.sun_dir[0] && q.sun_dir[1] == r.sun_dir[1] && q.sun_dir[2] == r.sun_dir[2] &&
         q.ray_noise == r.ray_noise && q.reflection_noise == r.reflection_noise &&
         q.refraction_noise == r.refraction_noise && q.max_ray_length == r.max_ray_length &&
         q.max_reflections == r.max_reflections && q.max_transparencies == r.max_transparencies &&
         q.color_only == r.color_only && q.atlas_rgba == r.atlas_rgba && q.atlas_size == r.atlas_size &&
         q.atlas_texture_size == r.atlas_texture_size;
}

// Frames [f0, f0 + nframes) of a batch whose per-launch params agree: the fewest launches that hold them
static int batch_run(vrt_ctx* ctx, int32_t nframes, const vrt_camera* cams, const vrt_params* p, int32_t row0,
                     int32_t rows, int32_t row_step, int32_t sh, int64_t pitch, uint32_t* const* d_cur_rgba8,
                     uint32_t* const* d_raw_rgba8, void* hip_stream) {
  Shard& s = ctx->sh[0];
  int per = nframes;  // frames per launch, from the first launch's tile count
  for (int f0 = 0; f0 < nframes; f0 += per) {
    // frame f0 of the batch is the launch's frame 0: its camera's argument block (vdiv_ok included)
    vrt::KArgs b = make_args(ctx, s, &cams[f0], p, row0, rows, row_step);
    const uint32_t ft = b.tiles;
    if (f0 == 0) {
      // a launch holds at most kOrderMaxTiles tiles (the tile order's and the deferred list's slot):
      // a larger batch is enqueued as the fewest consecutive launches that fit, of equal frame counts
      // (7 frames that fit 6 at a time: 4 + 3, not 6 + 1)
      const int fit = int(std::max<uint32_t>(1u, std::min<uint32_t>(uint32_t(nframes), kOrderMaxTiles / std::max(ft, 1u))));
      const int nlaunch = (nframes + fit - 1) / fit;
      per = (nframes + nlaunch - 1) / nlaunch;
    }
    const int nf = std::min(per, nframes - f0);
    b.row_blk_sh = sh;
    b.pitch = int32_t(pitch);
    b.alpha = 1.0f;  // frames of a batch are independent: no history is read
    b.prev = d_cur_rgba8[f0];
    b.cur = d_cur_rgba8[f0];
    b.raw = d_raw_rgba8 ? d_raw_rgba8[f0] : nullptr;
    b.time = p[f0].time;
    for (int f = 1; f < nf; ++f) {
      vrt::KArgs::FrameB& z = b.fb[f - 1];
      std::memcpy(z.inv_pv, cams[f0 + f].inv_pv, sizeof(z.inv_pv));
      z.time = p[f0 + f].time;
      z.cur = d_cur_rgba8[f0 + f];
      z.raw = d_raw_rgba8 ? d_raw_rgba8[f0 + f] : nullptr;
    }
    b.nframes = nf;
    b.frame_tiles = ft;
    b.tiles = ft * uint32_t(nf);
    hipEvent_t eb, ee;
    launch_timing_events(ctx, eb, ee);
    launch(ctx, s, b, nullptr, nullptr, nullptr, static_cast<hipStream_t>(hip_stream), eb, ee);
    VRT_HIP(ctx, hipGetLastError());
  }
  return VRT_OK;
}

int vrt_render_temporal_batch_async(vrt_ctx* ctx, int32_t nframes, const vrt_camera* cams, const vrt_params* p,
                                    int32_t row0, int32_t rows, int32_t row_step, int32_t row_block, int64_t pitch,
                                    uint32_t* const* d_cur_rgba8, uint32_t* const* d_raw_rgba8, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (nframes < 1 || nframes > vrt::kMaxBatch || !cams || !p || !d_cur_rgba8)
    return fail(ctx, VRT_ERR_INVALID, "nframes must be in [1, 8] with a camera, params and an output per frame");
  for (int f = 0; f < nframes; ++f) {
    const int st = check_render_args(ctx, &cams[f], &p[f]);
    if (st != VRT_OK) return st;
    if (!d_cur_rgba8[f]) return fail(ctx, VRT_ERR_INVALID, "null output");
    if (cams[f].width != cams[0].width || cams[f].height != cams[0].height)
      return fail(ctx, VRT_ERR_INVALID, "the frames of a batch share the image size");
  }
  int32_t sh = 0;
  int st = check_band(ctx, &cams[0], row0, rows, row_step, pitch, row_block, &sh);
  if (st != VRT_OK) return st;
  if (nframes > 1 && rows >= 8192) return fail(ctx, VRT_ERR_UNSUPPORTED, "frame batches need bands of < 8192 rows");
  if (rows == 0) return VRT_OK;
  // runs of consecutive frames whose per-launch params agree share a launch (the reference's
  // day/night cycle moves u_SunDir every frame, main.cpp:346-348, 397-399: such frames take a
  // launch each, in order on the stream)
  for (int f0 = 0; f0 < nframes;) {
    int f1 = f0 + 1;
    while (f1 < nframes && same_launch_params(p[f1], p[f0])) ++f1;
    st = batch_run(ctx, f1 - f0, cams + f0, p + f0, row0, rows, row_step, sh, pitch, d_cur_rgba8 + f0,
                   d_raw_rgba8 ? d_raw_rgba8 + f0 : nullptr, hip_stream);
    if (st != VRT_OK) return st;
    f0 = f1;
  }
  return VRT_OK;
}

int vrt_render_temporal_rows_pitched_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p,
                                           float alpha, int32_t row0, int32_t rows, int32_t row_step,
                                           int64_t pitch, const uint32_t* d_prev_rgba8, uint32_t* d_cur_rgba8,
                                           uint32_t* d_raw_rgba8, vrt_hit* d_out_hit, uint64_t* d_counters,
                                           void* hip_stream) {
  return vrt_render_temporal_blocks_pitched_async(ctx, cam, p, alpha, row0, rows, row_step, 1, pitch,
                                                  d_prev_rgba8, d_cur_rgba8, d_raw_rgba8, d_out_hit,
                                                  d_counters, hip_stream);
}

int vrt_render_temporal_rows_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, float alpha,
                                   int32_t row0, int32_t rows, int32_t row_step, const uint32_t* d_prev_rgba8,
                                   uint32_t* d_cur_rgba8, uint32_t* d_raw_rgba8, vrt_hit* d_out_hit,
                                   uint64_t* d_counters, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!cam) return fail(ctx, VRT_ERR_INVALID, "null camera");
  return vrt_render_temporal_rows_pitched_async(ctx, cam, p, alpha, row0, rows, row_step, cam->width,
                                                d_prev_rgba8, d_cur_rgba8, d_raw_rgba8, d_out_hit, d_counters,
                                                hip_stream);
}

}  // extern "C"
