// vrt_queries.cpp — queries on the resident volume, all on the first device: ray casts and pixel picks, shaded
// ray and pixel traces, the ID and depth pass (vrt_context.h). The filters that work on the ID pass's buffers are
// vrt_filters.cpp.
#include <algorithm>

#include "vrt_context.h"

using namespace vrt;

// ---- ID and depth pass (vrt_ids_kernels.h): what vrt_filters.cpp shares (vrt_context.h) ------------

int vrt::check_ids(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0, int32_t rows, int64_t pitch,
                   const void* ids, const void* depth, bool device) {
  if (!cam || !p) return fail(ctx, VRT_ERR_INVALID, "null camera or params");
  if (!ctx->sh[0].d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (const int st = check_image(ctx, cam); st != VRT_OK) return st;
  if (const int st = check_band(ctx, cam->width, cam->height, row0, rows, pitch); st != VRT_OK) return st;
  if (!ids) return fail(ctx, VRT_ERR_INVALID, "null id buffer");
  if (device && ((reinterpret_cast<uintptr_t>(ids) & 7u) != 0 || (reinterpret_cast<uintptr_t>(depth) & 3u) != 0))
    return fail(ctx, VRT_ERR_INVALID, "device id buffer must be 8-byte aligned, depth buffer 4-byte aligned");
  return VRT_OK;
}

// Whether the next ID pass launches the certified ID kernel: asked for, and the resident volume has the
// eight-octant skip layout its walk needs (the single layout, N = 1024 or vrt_set_skip_layout(1): the exact kernel)
bool vrt::ids_certified(const vrt_ctx* ctx) {
  const Shard& s = ctx->sh[0];
  return ctx->ids_cert_req == 1 && s.d_vox_pad && s.octants == 8;
}

int vrt::enqueue_ids(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0, int32_t rows,
                     int32_t pitch, vrt_pixel_id* d_ids, float* d_depth, hipStream_t st, uint32_t* d_n_exact) {
  Shard& s = ctx->sh[0];
  // the frame's argument block, as the frame launches fill it (launch): primary_ray reads it
  vrt::KArgs a = make_args(ctx, s, cam, p, row0, rows, 1);
  a.pitch = pitch;
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  vrt::launch_render_ids(a, s.d_vox_pad, d_ids, d_depth, st, eb, ee, ids_certified(ctx), d_n_exact);
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

extern "C" {

// ---- ray queries (vrt_query_kernels.h) ---------------------------------------------------------

// Arguments shared by the casts. Device buffers (the kernel's 16-byte loads and stores) must be
// 16-byte aligned; host buffers are only copied.
static int check_cast(vrt_ctx* ctx, const void* rays, int64_t count, int32_t mode, const void* hits, bool device) {
  if (!ctx->sh[0].d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (count < 0 || count > (int64_t(1) << 30)) return fail(ctx, VRT_ERR_INVALID, "ray count must be in [0, 2^30]");
  if (mode != VRT_CAST_NEAREST && mode != VRT_CAST_OCCLUSION) return fail(ctx, VRT_ERR_INVALID, "unknown cast mode");
  if (count > 0 && (!rays || !hits)) return fail(ctx, VRT_ERR_INVALID, "null ray or hit buffer");
  if (device && count > 0 && ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(hits)) & 15u) != 0)
    return fail(ctx, VRT_ERR_INVALID, "device ray and hit buffers must be 16-byte aligned");
  return VRT_OK;
}

// The argument block of a cast: ray_query_kernel reads the volume's fields only
static vrt::KArgs cast_args(const Shard& s) {
  vrt::KArgs a{};
  a.n = s.n;
  a.fn = float(s.n);
  a.ostride = octant_stride(s);
  return a;
}

// The synchronous queries' staging on the first device (the current one): `records` of 32 bytes in
// and out. The queries are synchronous, so no launch still reads buffers that are replaced here.
static int ensure_query_stage(vrt_ctx* ctx, size_t records) {
  static_assert(sizeof(vrt_ray) == 32 && sizeof(vrt_ray_hit) == 32, "query records are 32 bytes");
  if (ctx->d_query_in.cap >= records) return VRT_OK;
  const size_t cap = std::max<size_t>(std::max(records, 2 * ctx->d_query_in.cap), 4096);
  if (!stage_alloc_all(cap, ctx->d_query_in, ctx->d_query_out))
    return fail(ctx, VRT_ERR_OOM, "hipMalloc ray-query staging");
  return VRT_OK;
}

// `in` (host, in_bytes) to the staging, one query launch over `count` queries (shaded: launch_ray_trace
// of kind kTraceRays / kTracePixels, else launch_ray_query), the 32-byte records back to `out` (host); waits
static int run_query_staged(vrt_ctx* ctx, const vrt::KArgs& a, int32_t kind, bool shaded, const void* in,
                            size_t in_bytes, size_t count, void* out) {
  static_assert(sizeof(vrt_ray_color) == sizeof(vrt_ray_hit), "one staging for both record types");
  DeviceGuard guard;
  Shard& s = ctx->sh[0];
  VRT_HIP(ctx, hipSetDevice(s.device));
  const int st = ensure_query_stage(ctx, count);
  if (st != VRT_OK) return st;
  hipStream_t qs = main_stream(s);
  VRT_HIP(ctx, hipMemcpyAsync(ctx->d_query_in.p, in, in_bytes, hipMemcpyHostToDevice, qs));
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  if (shaded)
    vrt::launch_ray_trace(a, kind, s.d_vox_pad, ctx->d_query_in.p, uint32_t(count),
                          reinterpret_cast<vrt_ray_color*>(ctx->d_query_out.p), qs, eb, ee);
  else
    vrt::launch_ray_query(a, kind, s.d_vox_pad, ctx->d_query_in.p, uint32_t(count), ctx->d_query_out.p, qs, eb, ee);
  VRT_HIP(ctx, hipGetLastError());
  VRT_HIP(ctx, hipMemcpyAsync(out, ctx->d_query_out.p, count * sizeof(vrt_ray_hit), hipMemcpyDeviceToHost, qs));
  VRT_HIP(ctx, hipStreamSynchronize(qs));
  return VRT_OK;
}

int vrt_cast_rays_async(vrt_ctx* ctx, const vrt_ray* d_rays, int64_t count, int32_t mode, vrt_ray_hit* d_hits,
                        void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  const int st = check_cast(ctx, d_rays, count, mode, d_hits, true);
  if (st != VRT_OK || count == 0) return st;
  Shard& s = ctx->sh[0];
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  vrt::launch_ray_query(cast_args(s), mode, s.d_vox_pad, d_rays, uint32_t(count), d_hits,
                        static_cast<hipStream_t>(hip_stream), eb, ee);
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

int vrt_cast_rays(vrt_ctx* ctx, const vrt_ray* rays, int64_t count, int32_t mode, vrt_ray_hit* hits) {
  if (!ctx) return VRT_ERR_INVALID;
  const int st = check_cast(ctx, rays, count, mode, hits, false);
  if (st != VRT_OK || count == 0) return st;
  return run_query_staged(ctx, cast_args(ctx->sh[0]), mode, false, rays, size_t(count) * sizeof(vrt_ray),
                          size_t(count), hits);
}

int vrt_pick_pixels(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, const int32_t* pixels, int32_t count,
                    vrt_ray_hit* hits) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!cam || !p) return fail(ctx, VRT_ERR_INVALID, "null camera or params");
  Shard& s = ctx->sh[0];
  if (!s.d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (const int st = check_image(ctx, cam); st != VRT_OK) return st;
  if (count < 0) return fail(ctx, VRT_ERR_INVALID, "pixel count must be >= 0");
  if (count == 0) return VRT_OK;
  if (!pixels || !hits) return fail(ctx, VRT_ERR_INVALID, "null pixel or hit buffer");
  if (const int st = check_pixel_list(ctx, cam, pixels, count); st != VRT_OK) return st;
  // the frame's argument block, as the frame launches fill it (launch): primary_ray reads it
  vrt::KArgs a = make_args(ctx, s, cam, p, 0, cam->height, 1);
  return run_query_staged(ctx, a, vrt::kQueryPick, false, pixels, size_t(count) * 2 * sizeof(int32_t), size_t(count),
                          hits);
}

// ---- ID and depth pass (vrt_ids_kernels.h) -----------------------------------------------------

int vrt_render_ids_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0, int32_t rows,
                         int32_t pitch, vrt_pixel_id* d_ids, float* d_depth, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  const int st = check_ids(ctx, cam, p, row0, rows, pitch, d_ids, d_depth, true);
  if (st != VRT_OK || rows == 0) return st;
  return enqueue_ids(ctx, cam, p, row0, rows, pitch, d_ids, d_depth, static_cast<hipStream_t>(hip_stream));
}

int vrt_render_ids(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, vrt_pixel_id* ids, float* depth) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_ids(ctx, cam, p, 0, cam ? cam->height : 0, cam ? cam->width : 0, ids, depth, false);
  if (st != VRT_OK) return st;
  DeviceGuard guard;
  Shard& s = ctx->sh[0];
  VRT_HIP(ctx, hipSetDevice(s.device));
  const size_t px = size_t(cam->width) * size_t(cam->height);
  // the staging: synchronous calls only, so no launch still writes buffers that are replaced here
  if (ctx->d_ids_stage.cap < px) {
    if (!stage_alloc_all(px, ctx->d_ids_stage, ctx->d_depth_stage) || !ctx->d_ids_count.alloc(1)) {
      ctx->d_ids_stage.release();
      ctx->d_depth_stage.release();
      return fail(ctx, VRT_ERR_OOM, "hipMalloc ID pass staging");
    }
  }
  hipStream_t qs = main_stream(s);
  // the certified kernel counts its exact-path pixels into the context's word, zeroed here on the same stream;
  // the exact kernel (mode 0, or the single layout) takes every pixel and needs no counter
  const bool cert = ids_certified(ctx);
  uint32_t n_exact = 0;
  if (cert) VRT_HIP(ctx, hipMemsetAsync(ctx->d_ids_count.p, 0, sizeof(uint32_t), qs));
  st = enqueue_ids(ctx, cam, p, 0, cam->height, cam->width, ctx->d_ids_stage.p, depth ? ctx->d_depth_stage.p : nullptr, qs,
                   cert ? ctx->d_ids_count.p : nullptr);
  if (st != VRT_OK) return st;
  VRT_HIP(ctx, hipMemcpyAsync(ids, ctx->d_ids_stage.p, px * sizeof(vrt_pixel_id), hipMemcpyDeviceToHost, qs));
  if (depth) VRT_HIP(ctx, hipMemcpyAsync(depth, ctx->d_depth_stage.p, px * sizeof(float), hipMemcpyDeviceToHost, qs));
  if (cert) VRT_HIP(ctx, hipMemcpyAsync(&n_exact, ctx->d_ids_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, qs));
  VRT_HIP(ctx, hipStreamSynchronize(qs));
  ctx->ids_pixels = px;
  ctx->ids_deferred = cert ? n_exact : px;
  return VRT_OK;
}

int vrt_set_ids_certified(vrt_ctx* ctx, int32_t mode) {
  if (!ctx) return VRT_ERR_INVALID;
  if (mode != 0 && mode != 1) return fail(ctx, VRT_ERR_INVALID, "certified ID mode must be 0 or 1");
  ctx->ids_cert_req = mode;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_ids_certified(const vrt_ctx* ctx) {
  if (!ctx) return VRT_ERR_INVALID;
  return ids_certified(ctx) ? 1 : 0;
}

int vrt_ids_deferred(vrt_ctx* ctx, uint64_t* pixels, uint64_t* deferred) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!pixels || !deferred) return fail(ctx, VRT_ERR_INVALID, "null output");
  *pixels = ctx->ids_pixels;
  *deferred = ctx->ids_deferred;
  return VRT_OK;
}

// ---- shaded ray queries (vrt_trace_kernels.h) --------------------------------------------------

// The params of a trace call: max_reflections and max_transparencies in vrt_params' range 0..8 each (so
// the stack fits kMaxStack), as VRT_ERR_INVALID, then what the render calls check (check_render_args: the
// atlas rules, which upload a changed atlas as the render calls do). Last of a call's checks: a call that
// fails another check uploads nothing.
static int check_trace_params(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p) {
  constexpr int32_t kMaxDepth = (vrt::kMaxStack - 1) / 2;
  if (p->max_reflections < 0 || p->max_transparencies < 0 || p->max_reflections > kMaxDepth ||
      p->max_transparencies > kMaxDepth)
    return fail(ctx, VRT_ERR_INVALID, "max_reflections and max_transparencies must be in [0, 8]");
  return check_render_args(ctx, cam, p);
}

// Arguments shared by vrt_trace_rays*. Device buffers (the kernel's 16-byte loads and stores) must be
// 16-byte aligned; host buffers are only copied.
static int check_trace_rays(vrt_ctx* ctx, const void* rays, int64_t count, const vrt_params* p, const void* out,
                            bool device, const vrt_camera* dummy) {
  if (!p) return fail(ctx, VRT_ERR_INVALID, "null params");
  if (!ctx->sh[0].d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (count < 0 || count > (int64_t(1) << 30)) return fail(ctx, VRT_ERR_INVALID, "ray count must be in [0, 2^30]");
  if (count > 0 && (!rays || !out)) return fail(ctx, VRT_ERR_INVALID, "null ray or output buffer");
  if (device && count > 0 && ((reinterpret_cast<uintptr_t>(rays) | reinterpret_cast<uintptr_t>(out)) & 15u) != 0)
    return fail(ctx, VRT_ERR_INVALID, "device ray and output buffers must be 16-byte aligned");
  return check_trace_params(ctx, dummy, p);
}

// The rays form needs no camera: a 1 x 1 image whose matrix no lane reads
static vrt_camera trace_dummy_camera() {
  vrt_camera cam{};
  cam.width = cam.height = 1;
  return cam;
}

int vrt_trace_rays_async(vrt_ctx* ctx, const vrt_ray* d_rays, int64_t count, const vrt_params* p,
                         vrt_ray_color* d_out, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  const vrt_camera cam = trace_dummy_camera();
  const int st = check_trace_rays(ctx, d_rays, count, p, d_out, true, &cam);
  if (st != VRT_OK || count == 0) return st;
  Shard& s = ctx->sh[0];
  hipEvent_t eb, ee;
  launch_timing_events(ctx, eb, ee);
  vrt::launch_ray_trace(make_args(ctx, s, &cam, p, 0, 1, 1), vrt::kTraceRays, s.d_vox_pad, d_rays, uint32_t(count),
                        d_out, static_cast<hipStream_t>(hip_stream), eb, ee);
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

int vrt_trace_rays(vrt_ctx* ctx, const vrt_ray* rays, int64_t count, const vrt_params* p, vrt_ray_color* out) {
  if (!ctx) return VRT_ERR_INVALID;
  const vrt_camera cam = trace_dummy_camera();
  const int st = check_trace_rays(ctx, rays, count, p, out, false, &cam);
  if (st != VRT_OK || count == 0) return st;
  Shard& s = ctx->sh[0];
  return run_query_staged(ctx, make_args(ctx, s, &cam, p, 0, 1, 1), vrt::kTraceRays, true, rays,
                          size_t(count) * sizeof(vrt_ray), size_t(count), out);
}

int vrt_trace_pixels(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, const int32_t* pixels, int32_t count,
                     vrt_ray_color* out) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!cam || !p) return fail(ctx, VRT_ERR_INVALID, "null camera or params");
  Shard& s = ctx->sh[0];
  if (!s.d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (const int st = check_image(ctx, cam); st != VRT_OK) return st;
  if (count < 0) return fail(ctx, VRT_ERR_INVALID, "pixel count must be >= 0");
  if (count > 0 && (!pixels || !out)) return fail(ctx, VRT_ERR_INVALID, "null pixel or output buffer");
  int st = check_pixel_list(ctx, cam, pixels, count);
  if (st != VRT_OK) return st;
  st = check_trace_params(ctx, cam, p);
  if (st != VRT_OK || count == 0) return st;
  // the frame's argument block, as the frame launches fill it (launch): primary_ray reads it
  vrt::KArgs a = make_args(ctx, s, cam, p, 0, cam->height, 1);
  return run_query_staged(ctx, a, vrt::kTracePixels, true, pixels, size_t(count) * 2 * sizeof(int32_t),
                          size_t(count), out);
}

}  // extern "C"
