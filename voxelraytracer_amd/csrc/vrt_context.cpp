// vrt_context.cpp — a context's life and settings: create / destroy and the shards' resources, the checks the
// entry points share, the vrt_set_* / getter entry points, launch timing, the debug hooks that need a device,
// and the error string (vrt_context.h).
#include <cstring>
#include <vector>

#include "vrt_context.h"

namespace vrt {

static void shard_free(Shard& s) {
  (void)hipSetDevice(s.device);
  std::vector<void*> bufs = {(void*)s.d_vox, (void*)s.d_tmp, (void*)s.d_vox_pad, (void*)s.d_vstats,
                             (void*)s.d_cnt, (void*)s.d_cnt_rep, (void*)s.d_out, (void*)s.d_hit,
                             (void*)s.d_atlas, (void*)s.d_order_pool};
  for (OrderSlot& o : s.order) {
    bufs.push_back(o.defer);
    if (o.h_batches) (void)hipHostFree(o.h_batches);
    if (o.ev_last) (void)hipEventDestroy(o.ev_last);
  }
  for (int r = 0; r < kRing; ++r) {
    bufs.push_back(s.d_ring[r]);
    bufs.push_back(s.d_rawbuf[r]);
  }
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  std::vector<hipEvent_t> evs = {s.ev_gs};
  for (int q = 0; q < kParts; ++q) {
    evs.push_back(s.ev_kbeg[q]);
    evs.push_back(s.ev_kend[q]);
  }
  for (int l = 0; l < kLanes; ++l)
    for (int q = 0; q < kParts; ++q) evs.push_back(s.ev_done[l][q]);
  for (int r = 0; r < kRing; ++r) evs.push_back(s.ev_band_read[r]);
  for (hipEvent_t e : evs)
    if (e) (void)hipEventDestroy(e);
  for (int l = 0; l < kLanes; ++l)
    for (int q = 0; q < kParts; ++q)
      if (s.ls[l][q]) (void)hipStreamDestroy(s.ls[l][q]);
  if (s.gs) (void)hipStreamDestroy(s.gs);
  s = Shard();
}

static hipError_t shard_init(Shard& s, int device) {
  s.device = device;
  hipError_t e = hipSetDevice(device);
  int cus = 0;
  if (e == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
      cus > 0)
    s.wave_slots = uint32_t(cus) * 4u * 7u;
  const size_t rep_bytes = sizeof(unsigned long long) * vrt::kCntReplicas * VRT_CNT_COUNT;
  const size_t pool_words = size_t(kOrderSlots) * kOrderSlotWords;
  // ordering markers without timestamps (timing events make the command processor stamp and
  // flush around them: ~20 us gaps between the launches of a stream, measured)
  // HIP deals streams to its hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in creation order:
  // the lanes' first streams first, so that frames in flight land on distinct queues
  for (int q = 0; q < kParts; ++q)
    for (int l = 0; l < kLanes && e == hipSuccess; ++l) {
      e = hipStreamCreateWithFlags(&s.ls[l][q], hipStreamNonBlocking);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_done[l][q], hipEventDisableTiming);
    }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&s.gs, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev_gs, hipEventDisableTiming);
  for (int r = 0; r < kRing && e == hipSuccess; ++r)
    e = hipEventCreateWithFlags(&s.ev_band_read[r], hipEventDisableTiming);
  for (int q = 0; q < kParts && e == hipSuccess; ++q) {
    e = hipEventCreate(&s.ev_kbeg[q]);
    if (e == hipSuccess) e = hipEventCreate(&s.ev_kend[q]);
  }
  if (e == hipSuccess) e = hipMalloc(&s.d_cnt, sizeof(unsigned long long) * VRT_CNT_COUNT);
  if (e == hipSuccess) e = hipMalloc(&s.d_cnt_rep, rep_bytes);
  if (e == hipSuccess) e = hipMemset(s.d_cnt_rep, 0, rep_bytes);
  if (e == hipSuccess) e = hipMalloc(&s.d_order_pool, pool_words * sizeof(uint32_t));
  for (int i = 0; i < kOrderSlots && e == hipSuccess; ++i) s.order[i].d = s.d_order_pool + size_t(i) * kOrderSlotWords;
  return e;
}

// The image size limits of every entry point that takes a camera or an image size
int check_image(vrt_ctx* ctx, int32_t width, int32_t height) {
  if (width <= 0 || height <= 0 || width > 32768 || height > 32768) return fail(ctx, VRT_ERR_INVALID, "bad image size");
  return VRT_OK;
}
int check_image(vrt_ctx* ctx, const vrt_camera* cam) { return check_image(ctx, cam->width, cam->height); }

// A band of rows [row0, row0 + rows) of a width x height image in buffers of `pitch` pixels per row (the ID pass,
// the reprojection, a spatial pass). pitch_first: which of the two a call with both wrong reports (the spatial
// pass has always named the pitch, the others the band)
int check_band(vrt_ctx* ctx, int32_t width, int32_t height, int32_t row0, int32_t rows, int64_t pitch, bool pitch_first) {
  const bool bad_band = rows < 0 || row0 < 0 || int64_t(row0) + rows > height, bad_pitch = pitch < width;
  if (bad_pitch && (pitch_first || !bad_band)) return fail(ctx, VRT_ERR_INVALID, "row pitch must be >= the image width");
  if (bad_band) return fail(ctx, VRT_ERR_INVALID, "row band outside the image");
  return VRT_OK;
}

// A list of `count` {px, py} pairs (vrt_pick_pixels, vrt_trace_pixels): every pixel inside the image
int check_pixel_list(vrt_ctx* ctx, const vrt_camera* cam, const int32_t* pixels, int32_t count) {
  for (int32_t i = 0; i < count; ++i)
    if (pixels[2 * i] < 0 || pixels[2 * i] >= cam->width || pixels[2 * i + 1] < 0 || pixels[2 * i + 1] >= cam->height)
      return fail(ctx, VRT_ERR_INVALID, "pixel outside the image");
  return VRT_OK;
}

int check_render_args(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p) {
  if (!cam || !p) return fail(ctx, VRT_ERR_INVALID, "null camera or params");
  if (!ctx->sh[0].d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (const int st = check_image(ctx, cam); st != VRT_OK) return st;
  if (!p->color_only) {  // textured mode: the context's atlas (uploaded here when it changes)
    const size_t abytes = p->atlas_size > 0 ? size_t(p->atlas_size) * size_t(p->atlas_size) * 4 : 0;
    if (p->atlas_rgba && (p->atlas_size != ctx->sh[0].atlas_size || abytes != ctx->atlas_host.size() ||
                          std::memcmp(p->atlas_rgba, ctx->atlas_host.data(), abytes) != 0)) {
      const int st = upload_atlas(ctx, p->atlas_rgba, p->atlas_size);
      if (st != VRT_OK) return st;
    }
    if (!ctx->sh[0].d_atlas || p->atlas_size != ctx->sh[0].atlas_size)
      return fail(ctx, VRT_ERR_INVALID, "textured mode needs an atlas of atlas_size (vrt_upload_atlas)");
    if (p->atlas_texture_size <= 0) return fail(ctx, VRT_ERR_INVALID, "atlas_texture_size must be > 0");
  }
  if (p->max_reflections < 0 || p->max_transparencies < 0 ||
      p->max_reflections + p->max_transparencies + 1 > vrt::kMaxStack)
    return fail(ctx, VRT_ERR_UNSUPPORTED, "max_reflections + max_transparencies must be <= 16");
  return VRT_OK;
}

static int create(const std::vector<int>& devs, vrt_ctx** out) {
  if (!out) return VRT_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return VRT_ERR_DEVICE;
  if (devs.empty() || devs.size() > 64) return VRT_ERR_INVALID;
  for (int d : devs)
    if (d < 0 || d >= count) return VRT_ERR_INVALID;
  DeviceGuard guard;
  vrt_ctx* c = new vrt_ctx();
  c->sh.resize(devs.size());
  for (size_t j = 0; j < devs.size(); ++j) {
    if (shard_init(c->sh[j], devs[j]) != hipSuccess) {
      vrt_destroy(c);
      return VRT_ERR_DEVICE;
    }
    for (size_t i = 0; i < j; ++i)
      if (devs[i] == devs[j]) c->distinct = false;
  }
  if (hipSetDevice(devs[0]) != hipSuccess ||
      hipEventCreateWithFlags(&c->ev_gathered, hipEventDisableTiming) != hipSuccess ||
      [&] {
        for (hipEvent_t& e : c->ev_consumed)
          if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return true;
        for (hipEvent_t& e : c->ev_slot)
          if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return true;
        return false;
      }()) {
    vrt_destroy(c);
    return VRT_ERR_DEVICE;
  }
  if (devs.size() > 1 && c->distinct) {  // one communicator per device, this process owns them all
    c->comms.resize(devs.size());
    if (ncclCommInitAll(c->comms.data(), int(devs.size()), devs.data()) != ncclSuccess) {
      c->comms.clear();
      vrt_destroy(c);
      return VRT_ERR_DEVICE;
    }
  }
  *out = c;
  return VRT_OK;
}

}  // namespace vrt

using namespace vrt;

extern "C" {

int vrt_create(uint32_t device_mask, vrt_ctx** out) {
  std::vector<int> devs;
  for (int d = 0; d < 32; ++d)
    if (device_mask & (1u << d)) devs.push_back(d);
  if (devs.empty()) {
    if (out) *out = nullptr;
    return VRT_ERR_INVALID;
  }
  return create(devs, out);
}

int vrt_create_devices(const int32_t* devices, int32_t count, vrt_ctx** out) {
  if (!devices || count < 1) {
    if (out) *out = nullptr;
    return VRT_ERR_INVALID;
  }
  return create(std::vector<int>(devices, devices + count), out);
}

void vrt_destroy(vrt_ctx* c) {
  if (!c) return;
  DeviceGuard guard;
  for (ncclComm_t cm : c->comms) (void)ncclCommDestroy(cm);
  if (!c->rank_comms.empty()) {
    (void)hipSetDevice(c->sh[0].device);
    (void)hipDeviceSynchronize();  // no gather still runs on them
    for (ncclComm_t cm : c->rank_comms) (void)ncclCommDestroy(cm);
  }
  if (!c->sh.empty()) {
    (void)hipSetDevice(c->sh[0].device);
    if (c->d_gather) (void)hipFree(c->d_gather);
    for (uint32_t* f : c->d_frames)
      if (f) (void)hipFree(f);
    for (hipEvent_t e : c->ev_consumed)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_slot)
      if (e) (void)hipEventDestroy(e);
    if (c->ev_gathered) (void)hipEventDestroy(c->ev_gathered);
    if (c->ev_rp_beg) (void)hipEventDestroy(c->ev_rp_beg);
    if (c->ev_rp_end) (void)hipEventDestroy(c->ev_rp_end);
    if (!c->lt_ev.empty()) (void)hipDeviceSynchronize();
    for (hipEvent_t e : c->lt_ev) (void)hipEventDestroy(e);
  }
  const int first = c->sh.empty() ? -1 : c->sh[0].device;
  for (Shard& s : c->sh) shard_free(s);
  if (first >= 0) (void)hipSetDevice(first);  // the stagings (Stage) release themselves on their device
  delete c;
}

int vrt_device_count(const vrt_ctx* ctx) { return ctx ? int(ctx->sh.size()) : VRT_ERR_INVALID; }

int vrt_device_ordinal(const vrt_ctx* ctx, int32_t i) {
  if (!ctx || i < 0 || size_t(i) >= ctx->sh.size()) return -1;
  return ctx->sh[size_t(i)].device;
}

const char* vrt_last_error(const vrt_ctx* c) { return c ? c->err.c_str() : "null context"; }

int vrt_set_skip_layout(vrt_ctx* ctx, int32_t octants) {
  if (!ctx) return VRT_ERR_INVALID;
  if (octants != 0 && octants != 1 && octants != 8)
    return fail(ctx, VRT_ERR_INVALID, "skip layout must be 0 (auto), 1 or 8");
  ctx->layout_req = octants;
  return VRT_OK;
}

int vrt_set_launch_timing(vrt_ctx* ctx, int32_t launches) {
  if (!ctx) return VRT_ERR_INVALID;
  if (launches < 0 || launches > (1 << 20)) return fail(ctx, VRT_ERR_INVALID, "launches must be in [0, 2^20]");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  if (!ctx->lt_ev.empty()) VRT_HIP(ctx, hipDeviceSynchronize());  // no launch still records into them
  for (hipEvent_t e : ctx->lt_ev) (void)hipEventDestroy(e);
  ctx->lt_ev.clear();
  ctx->lt_used = 0;
  for (int32_t i = 0; i < 2 * launches; ++i) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return fail(ctx, VRT_ERR_DEVICE, "hipEventCreate (launch timing)");
    ctx->lt_ev.push_back(e);
  }
  ctx->err.clear();
  return VRT_OK;
}

int vrt_launch_timing(vrt_ctx* ctx, double* total_ms, uint64_t* launches) {
  if (!ctx || !total_ms || !launches) return VRT_ERR_INVALID;
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  double total = 0.0;
  for (size_t i = 0; i + 1 < ctx->lt_used; i += 2) {
    VRT_HIP(ctx, hipEventSynchronize(ctx->lt_ev[i + 1]));
    float ms = 0.0f;
    VRT_HIP(ctx, hipEventElapsedTime(&ms, ctx->lt_ev[i], ctx->lt_ev[i + 1]));
    total += ms;
  }
  *total_ms = total;
  *launches = ctx->lt_used / 2;
  ctx->lt_used = 0;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_set_tile_order(vrt_ctx* ctx, int32_t on) {
  if (!ctx) return VRT_ERR_INVALID;
  if (on < 0 || on > 2) return fail(ctx, VRT_ERR_INVALID, "tile order must be 0, 1 or 2");
  ctx->tile_order = on;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_set_exact_pass(vrt_ctx* ctx, int32_t on) {
  if (!ctx) return VRT_ERR_INVALID;
  if (on < 0 || on > 2) return fail(ctx, VRT_ERR_INVALID, "exact pass must be 0, 1 or 2");
  ctx->exact_pass = on;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_set_certified(vrt_ctx* ctx, int32_t mode) {
  if (!ctx) return VRT_ERR_INVALID;
  if (mode < -1 || mode > 1) return fail(ctx, VRT_ERR_INVALID, "certified mode must be -1, 0 or 1");
  ctx->cert_req = mode;
  return VRT_OK;
}

int vrt_certified(const vrt_ctx* ctx) {
  if (!ctx) return VRT_ERR_INVALID;
  const Shard& s = ctx->sh[0];
  return s.octants == 8 && ctx->cert_req >= 0 && (ctx->cert_req > 0 || s.cert_auto || ctx->tree_req != 0) ? 1 : 0;
}

int vrt_set_cert_trees(vrt_ctx* ctx, int32_t on) {
  if (!ctx) return VRT_ERR_INVALID;
  if (on < 0 || on > 2) return fail(ctx, VRT_ERR_INVALID, "certified trees must be 0, 1 or 2");
  ctx->tree_req = on;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_volume_octants(const vrt_ctx* ctx) {
  if (!ctx) return VRT_ERR_INVALID;
  return ctx->sh[0].d_vox_pad ? ctx->sh[0].octants : 0;
}

int vrt_debug_fast_math(vrt_ctx* ctx, uint64_t* out) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!out) return fail(ctx, VRT_ERR_INVALID, "null output");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  unsigned long long c[7];
  const int st = vrt::run_fast_math_check(c);
  if (st != VRT_OK) return fail(ctx, st, "vrt_debug_fast_math");
  for (int i = 0; i < 7; ++i) out[i] = c[i];
  return VRT_OK;
}

int vrt_debug_pow_forms(vrt_ctx* ctx, uint64_t* out) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!out) return fail(ctx, VRT_ERR_INVALID, "null output");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  unsigned long long c[6];
  const int st = vrt::run_pow_forms_check(c);
  if (st != VRT_OK) return fail(ctx, st, "vrt_debug_pow_forms");
  for (int i = 0; i < 6; ++i) out[i] = c[i];
  return VRT_OK;
}

int vrt_debug_randomize(vrt_ctx* ctx, const float* dir, const float* pos, int32_t n, float randomness,
                        float seed, float* out) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!dir || !pos || !out || n < 0) return fail(ctx, VRT_ERR_INVALID, "null buffer or n < 0");
  if (n == 0) return VRT_OK;
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  const size_t bytes = size_t(n) * 3 * sizeof(float);
  float *d_dir = nullptr, *d_pos = nullptr, *d_out = nullptr;
  if (hipMalloc(&d_dir, bytes) != hipSuccess || hipMalloc(&d_pos, bytes) != hipSuccess ||
      hipMalloc(&d_out, bytes) != hipSuccess) {
    (void)hipFree(d_dir);
    (void)hipFree(d_pos);
    return fail(ctx, VRT_ERR_OOM, "hipMalloc");
  }
  hipError_t e = hipMemcpy(d_dir, dir, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_pos, pos, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    vrt::launch_randomize(d_dir, d_pos, n, randomness, seed, d_out, nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_dir);
  (void)hipFree(d_pos);
  (void)hipFree(d_out);
  if (e != hipSuccess) return hip_fail(ctx, e, "vrt_debug_randomize");
  return VRT_OK;
}

int vrt_debug_cert_walks(vrt_ctx* ctx, const void* rays, int64_t count, int32_t kind, void* out) {
  if (!ctx) return VRT_ERR_INVALID;
  const Shard& s = ctx->sh[0];
  if (!s.d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (s.octants != 8) return fail(ctx, VRT_ERR_UNSUPPORTED, "certified walks need the eight-octant skip layout");
  if (kind < 0 || kind > 3) return fail(ctx, VRT_ERR_INVALID, "walk kind must be 0, 1, 2 or 3");
  if (count < 0 || count > (int64_t(1) << 24)) return fail(ctx, VRT_ERR_INVALID, "ray count must be in [0, 2^24]");
  if (count == 0) return VRT_OK;
  if (!rays || !out) return fail(ctx, VRT_ERR_INVALID, "null ray or result buffer");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(s.device));
  const size_t bytes = size_t(count) * 32u;  // a ray and a result are 32 bytes each
  void *d_in = nullptr, *d_out = nullptr;
  if (hipMalloc(&d_in, bytes) != hipSuccess || hipMalloc(&d_out, bytes) != hipSuccess) {
    (void)hipFree(d_in);
    return fail(ctx, VRT_ERR_OOM, "hipMalloc");
  }
  hipError_t e = hipMemcpy(d_in, rays, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    vrt::KArgs a{};  // the kernel reads the volume's fields only
    a.n = s.n;
    a.fn = float(s.n);
    a.ostride = octant_stride(s);
    vrt::launch_cert_walks_debug(a, kind, s.d_vox_pad, d_in, uint32_t(count), d_out, nullptr);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  if (e != hipSuccess) return hip_fail(ctx, e, "vrt_debug_cert_walks");
  return VRT_OK;
}

int vrt_debug_collectives(vrt_ctx* ctx) {
  if (!ctx) return VRT_ERR_INVALID;
  if (ctx->sh.size() != 1 || !ctx->comms.empty())
    return fail(ctx, VRT_ERR_INVALID, "vrt_debug_collectives: a one-device context without communicators");
  DeviceGuard guard;
  int dev = ctx->sh[0].device;
  ncclComm_t comm = nullptr;
  VRT_NCCL(ctx, ncclCommInitAll(&comm, 1, &dev));
  ctx->comms.push_back(comm);
  ctx->coll1 = true;
  ctx->hist_w = ctx->hist_h = 0;  // the next frame allocates the assembled-frame ring
  ctx->err.clear();
  return VRT_OK;
}

}  // extern "C"
