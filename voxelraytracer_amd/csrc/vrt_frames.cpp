// vrt_frames.cpp — whole frames: the history ring and the lanes, one frame's launches on every device
// (launch_frame), staging to the host and the gather to the first device, the vrt_render* frame entry points,
// and the rank communicator / pack / assemble entry points of one-process-per-GPU jobs (vrt_context.h).
#include <algorithm>
#include <cstring>
#include <vector>

#include "vrt_context.h"

namespace vrt {

// Whole-frame band buffers of every device for a W x H frame (history black on (re)creation):
// the ring of filtered bands and the ring of raw bands; with several devices, the first device's
// ring of assembled frames.
static int ensure_history(vrt_ctx* ctx, int32_t w, int32_t h) {
  if (w == ctx->hist_w && h == ctx->hist_h) return VRT_OK;
  const int32_t k = int32_t(ctx->sh.size());
  const size_t pixels = size_t(band_cap(h, k)) * size_t(w);
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    VRT_HIP(ctx, hipDeviceSynchronize());  // nothing may still read the old buffers
    if (pixels > s.hist_pixels) {
      for (int r = 0; r < kRing; ++r)
        for (uint32_t** b : {&s.d_ring[r], &s.d_rawbuf[r]}) {
          if (*b) (void)hipFree(*b);
          *b = nullptr;
        }
      s.hist_pixels = 0;
      for (int r = 0; r < kRing; ++r)
        for (uint32_t** b : {&s.d_ring[r], &s.d_rawbuf[r]})
          if (hipMalloc(b, pixels * 4) != hipSuccess) return fail(ctx, VRT_ERR_OOM, "hipMalloc history buffers");
      s.hist_pixels = pixels;
    }
    for (int r = 0; r < kRing; ++r) {
      VRT_HIP(ctx, hipMemset(s.d_ring[r], 0, pixels * 4));
      VRT_HIP(ctx, hipMemset(s.d_rawbuf[r], 0, pixels * 4));
      s.band_read_valid[r] = false;
    }
    // hipMemset of device memory does not wait for the fill, and the lane streams are non-blocking
    // (not ordered after the null stream): without this wait a fill could land after the first
    // frame's pixels (black rows in a fresh context's first 4K frame, now and then)
    VRT_HIP(ctx, hipDeviceSynchronize());
    for (int l = 0; l < kLanes; ++l) s.lane_parts[l] = 0;
    for (int r = 0; r < kRing; ++r) s.slot_reader[r] = 0;
  }
  if (k > 1 || ctx->coll1) {
    VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
    for (uint32_t*& f : ctx->d_frames) {
      if (f) (void)hipFree(f);
      f = nullptr;
      if (hipMalloc(&f, size_t(w) * size_t(h) * 4) != hipSuccess) return fail(ctx, VRT_ERR_OOM, "hipMalloc frames");
    }
  }
  ctx->hist_w = w;
  ctx->hist_h = h;
  ctx->fk = 0;
  ctx->reset_pending = false;
  for (bool& v : ctx->raw_is_cur) v = false;
  for (bool& v : ctx->consumed_valid) v = false;
  for (bool& v : ctx->slot_valid) v = false;
  ctx->frame_stream = nullptr;
  return VRT_OK;
}

// st waits for every launch of lane l's last frame except the one on st itself (stream order)
static int wait_lane(vrt_ctx* ctx, Shard& s, int l, hipStream_t st) {
  for (int r = 0; r < s.lane_parts[l]; ++r)
    if (s.ls[l][r] != st) VRT_HIP(ctx, hipStreamWaitEvent(st, s.ev_done[l][r], 0));
  return VRT_OK;
}

// Launch one whole frame on every device, on lane g = fk % kLanes: band j as nparts launches on
// the lane's streams — one exact-instance launch when counting or writing hit records; one launch
// when `overlap` (device-output frames, which overlap each other) and the frame does not read its
// history; else kParts interleaved parts, whose launches fill each other's tails. rgba8: the
// temporal path from the history (ring[(fk-1) % kRing], or after vrt_history_reset the last raw
// frame) into ring[fk % kRing] (+ the raw band when u_Alpha != 1: at u_Alpha = 1 the filtered
// frame is the quantised frame); else the float band into d_out (+ d_hit). Every launch records
// its lane's done event; cross-lane ordering only where buffers are shared:
//  - the lane's previous frame had another layout: its launches on the other streams (same slot);
//  - the frame reads its history (u_Alpha != 1): frame fk-1's launches (its slot, other lane);
//  - a frame read this slot as its history: its lane's last launches (WAR; that lane's later
//    frames end after it);
//  - a device-output gather of frame fk-4 read this slot: its gather stream;
// timing: device timestamps of every launch (vrt_stats.kernel_ms; synchronous calls only).
struct FrameMode {
  bool rgba8 = false, hits = false, counting = false, timing = false, overlap = false, one_part = false;
};
static int launch_frame(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, float alpha, FrameMode m) {
  const int32_t k = int32_t(ctx->sh.size()), w = cam->width, h = cam->height;
  const uint64_t f = ctx->fk;
  const int g = int(f % kLanes), slot = int(f % kRing), pslot = int((f + kRing - 1) % kRing);
  // the kernel reads the history iff u_Alpha != 1 (store_pixel, vrt_render.hip)
  const bool hist = m.rgba8 && alpha != 1.0f;
  const bool single = m.counting || m.hits;  // one counter replica set: one counted launch
  // one_part: device-output frames consumed on their own stream (vrt_frame_stream)
  // k > 1: one launch per block-cyclic band (a band's blocks are not split into parts)
  // a synchronous whole frame that lone_defers: one launch (certified pass + exact pass)
  const bool lone = !m.overlap && !single && !hist && k == 1 &&
                    lone_defers(ctx, ctx->sh[0], make_args(ctx, ctx->sh[0], cam, p, 0, h, 1));
  const int nparts = single || m.one_part || (m.overlap && !hist) || lone || k > 1 ? 1 : kParts;
  LaunchMode lm;
  lm.allow_defer = m.overlap;
  lm.lone = lone;
  for (int32_t j = 0; j < k; ++j) {
    Shard& s = ctx->sh[j];
    VRT_HIP(ctx, hipSetDevice(s.device));
    for (int q = 0; q < kParts; ++q) s.timed[q] = false;
    const int32_t hb = band_rows(h, k, j);
    if (hb == 0) {
      s.lane_parts[g] = 0;
      continue;
    }
    int st;
    for (int q = 0; q < nparts; ++q) {
      hipStream_t sq = s.ls[g][q];
      if (s.lane_parts[g] != nparts && (st = wait_lane(ctx, s, g, sq)) != VRT_OK) return st;
      if (m.rgba8 && f > 0) {
        const int pg = int((f - 1) % kLanes);
        if (hist) {  // part q's history rows: frame f-1's launch with the same rows, or all of them
          if (s.lane_parts[pg] == nparts) VRT_HIP(ctx, hipStreamWaitEvent(sq, s.ev_done[pg][q], 0));
          else if ((st = wait_lane(ctx, s, pg, sq)) != VRT_OK) return st;
        }
      }
      if (m.rgba8 && s.slot_reader[slot] > 0 && (st = wait_lane(ctx, s, s.slot_reader[slot] - 1, sq)) != VRT_OK)
        return st;
      if (m.rgba8 && s.band_read_valid[slot]) VRT_HIP(ctx, hipStreamWaitEvent(sq, s.ev_band_read[slot], 0));
    }
    if (m.rgba8) s.band_read_valid[slot] = false;
    if (m.counting)
      VRT_HIP(ctx, hipMemsetAsync(s.d_cnt, 0, sizeof(unsigned long long) * VRT_CNT_COUNT, s.ls[g][0]));
    const uint32_t* hsrc = ctx->reset_pending && !ctx->raw_is_cur[pslot] ? s.d_rawbuf[pslot] : s.d_ring[pslot];
    for (int q = 0; q < nparts; ++q) {
      const BandGeom bg = block_band(h, k, frame_block(k), j);
      const PartRows pr = nparts == 1 ? PartRows{bg.row0, bg.rows, bg.row_step, 0} : part_rows(h, k, kParts, j, q);
      if (pr.rows == 0) {
        VRT_HIP(ctx, hipEventRecord(s.ev_done[g][q], s.ls[g][q]));
        continue;
      }
      vrt::KArgs a = make_args(ctx, s, cam, p, pr.row0, pr.rows, pr.row_step);
      a.row_blk_sh = nparts == 1 ? bg.sh : 0;
      a.pitch = int32_t(int64_t(w) * nparts);
      const size_t off = size_t(pr.band_row0) * size_t(w);
      s.timed[q] = m.timing;
      hipEvent_t kb = m.timing ? s.ev_kbeg[q] : nullptr, ke = m.timing ? s.ev_kend[q] : nullptr;
      if (m.rgba8) {
        a.alpha = alpha;
        a.prev = hsrc + off;
        a.cur = s.d_ring[slot] + off;
        a.raw = hist ? s.d_rawbuf[slot] + off : nullptr;
        launch(ctx, s, a, nullptr, nullptr, m.counting ? s.d_cnt : nullptr, s.ls[g][q], kb, ke, lm);
      } else {
        launch(ctx, s, a, s.d_out + off, m.hits ? s.d_hit + off : nullptr, m.counting ? s.d_cnt : nullptr,
               s.ls[g][q], kb, ke, lm);
      }
      VRT_HIP(ctx, hipGetLastError());
      VRT_HIP(ctx, hipEventRecord(s.ev_done[g][q], s.ls[g][q]));
    }
    s.lane_parts[g] = nparts;
    if (m.rgba8) {
      s.slot_reader[slot] = 0;
      if (hist) s.slot_reader[pslot] = g + 1;
    }
  }
  if (m.rgba8) {
    ctx->raw_is_cur[slot] = !hist;
    ctx->reset_pending = false;
  }
  return VRT_OK;
}

// Wait for every device, then fill stats: kernel_ms = the slowest device's span from its first
// launch's start to its last launch's end (device timestamps: the GPU time of the frame, as
// GL_TIME_ELAPSED measured the draw); counters summed.
static int finish_frame(vrt_ctx* ctx, vrt_stats* stats, bool counting) {
  float ms_max = 0.0f;
  unsigned long long tot[VRT_CNT_COUNT] = {0};
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    for (int l = 0; l < kLanes; ++l)
      for (int q = 0; q < kParts; ++q) VRT_HIP(ctx, hipStreamSynchronize(s.ls[l][q]));
    VRT_HIP(ctx, hipStreamSynchronize(s.gs));
    if (stats) {
      int first = -1;
      for (int q = 0; q < kParts; ++q)
        if (s.timed[q] && first < 0) first = q;
      if (first >= 0) {  // times relative to the first launch's start (may be negative)
        float lo = 0.0f, hi = 0.0f;
        for (int q = 0; q < kParts; ++q) {
          if (!s.timed[q]) continue;
          float b = 0.0f, e = 0.0f;
          VRT_HIP(ctx, hipEventElapsedTime(&b, s.ev_kbeg[first], s.ev_kbeg[q]));
          VRT_HIP(ctx, hipEventElapsedTime(&e, s.ev_kbeg[first], s.ev_kend[q]));
          lo = std::min(lo, b);
          hi = std::max(hi, e);
        }
        ms_max = std::max(ms_max, hi - lo);
      }
    }
    if (counting) {
      unsigned long long c[VRT_CNT_COUNT];
      VRT_HIP(ctx, hipMemcpy(c, s.d_cnt, sizeof(c), hipMemcpyDeviceToHost));
      for (int q = 0; q < VRT_CNT_COUNT; ++q) tot[q] += c[q];
    }
  }
  if (stats) {
    stats->kernel_ms = ms_max;
    if (counting)
      for (int q = 0; q < VRT_CNT_COUNT; ++q) stats->counters[q] = tot[q];
  }
  return VRT_OK;
}

// Pinned host staging of synchronous frames, at least `bytes` (portable: every device's DMA
// engine writes it directly, so the k band copies run in parallel)
int ensure_stage(vrt_ctx* ctx, size_t bytes) {
  if (ctx->h_stage.cap >= bytes) return VRT_OK;
  if (!ctx->h_stage.alloc(bytes)) return fail(ctx, VRT_ERR_OOM, "hipHostMalloc staging");
  return VRT_OK;
}

// Band j's rows (band row r = frame row j + r*k) into their frame rows of the pinned staging
// buffer at byte offset stage_off: one strided DMA per device on its own link, after every launch
// of the frame on lane g. The caller copies the staged frame out after finish_frame.
static int stage_bands(vrt_ctx* ctx, int g, int32_t w, int32_t h, const void* const* bands, size_t elem,
                size_t stage_off) {
  const int32_t k = int32_t(ctx->sh.size());
  for (int32_t j = 0; j < k; ++j) {
    Shard& s = ctx->sh[j];
    BandCopy bc[2];
    const int nc = band_copies(w, h, k, frame_block(k), j, elem, bc);
    if (nc == 0) continue;
    VRT_HIP(ctx, hipSetDevice(s.device));
    int st = wait_lane(ctx, s, g, s.ls[g][0]);
    if (st != VRT_OK) return st;
    for (int c = 0; c < nc; ++c)
      VRT_HIP(ctx, hipMemcpy2DAsync(ctx->h_stage.p + stage_off + bc[c].dst_off, bc[c].dst_pitch,
                                    static_cast<const char*>(bands[j]) + bc[c].src_off, bc[c].src_pitch, bc[c].width,
                                    bc[c].rows, hipMemcpyDeviceToHost, s.ls[g][0]));
  }
  return VRT_OK;
}

// Several devices (or the one-device RCCL rehearsal): frame f's bands (launched on lane g) to the
// first device — ncclGather over xGMI on every device's gather stream, or device-to-device copies
// when a device repeats — then placed into their rows of d_frames[slot] on the first device's
// gather stream; ev_gathered marks the assembled frame.
static int gather_frame(vrt_ctx* ctx, int32_t w, int32_t h, int slot, int g, const uint32_t** d_frame) {
  const int32_t k = int32_t(ctx->sh.size());
  Shard& root = ctx->sh[0];
  int st;
  const int32_t cap = band_cap(h, k);
  const size_t row = size_t(w) * 4;
  const uint32_t* src[64];
  if (ctx->distinct) {  // RCCL gather of the equal-size bands to the first device over xGMI
    if (!ctx->d_gather || size_t(k) * size_t(cap) * size_t(w) > ctx->hist_pixels_gather) {
      VRT_HIP(ctx, hipDeviceSynchronize());
      if (ctx->d_gather) (void)hipFree(ctx->d_gather);
      ctx->d_gather = nullptr;
      ctx->hist_pixels_gather = 0;
      const size_t need = size_t(k) * size_t(cap) * size_t(w);
      if (hipMalloc(&ctx->d_gather, need * 4) != hipSuccess) return fail(ctx, VRT_ERR_OOM, "hipMalloc gather");
      ctx->hist_pixels_gather = need;
    }
    for (int32_t j = 0; j < k; ++j) {  // each device's gather stream after its band's launches
      Shard& s = ctx->sh[j];
      VRT_HIP(ctx, hipSetDevice(s.device));
      if ((st = wait_lane(ctx, s, g, s.gs)) != VRT_OK) return st;
    }
    VRT_NCCL(ctx, ncclGroupStart());
    for (int32_t j = 0; j < k; ++j) {
      Shard& s = ctx->sh[j];
      (void)hipSetDevice(s.device);
      const ncclResult_t r = ncclGather(s.d_ring[slot], j == 0 ? ctx->d_gather : nullptr, size_t(cap) * row,
                                        ncclUint8, 0, ctx->comms[j], s.gs);
      if (r != ncclSuccess) {
        (void)ncclGroupEnd();
        return nccl_fail(ctx, r, "ncclGather(bands)");
      }
    }
    VRT_NCCL(ctx, ncclGroupEnd());
    for (int32_t j = 0; j < k; ++j) {  // the band's next writer (frame f + kRing) waits for this
      Shard& s = ctx->sh[j];
      VRT_HIP(ctx, hipSetDevice(s.device));
      VRT_HIP(ctx, hipEventRecord(s.ev_band_read[slot], s.gs));
      s.band_read_valid[slot] = true;
    }
    for (int32_t j = 0; j < k; ++j) src[j] = ctx->d_gather + size_t(j) * cap * w;
  } else {  // a device repeats: copy the bands device to device on the first device's stream
    VRT_HIP(ctx, hipSetDevice(root.device));
    for (int32_t j = 0; j < k; ++j)
      for (int q = 0; q < ctx->sh[j].lane_parts[g]; ++q)
        VRT_HIP(ctx, hipStreamWaitEvent(root.gs, ctx->sh[j].ev_done[g][q], 0));
    for (int32_t j = 0; j < k; ++j) src[j] = ctx->sh[j].d_ring[slot];
  }
  VRT_HIP(ctx, hipSetDevice(root.device));
  uint32_t* out = ctx->d_frames[slot];
  if (ctx->distinct) {  // the gathered bands, cap rows apart, into their frame rows: one kernel
    vrt::launch_assemble_blocks(ctx->d_gather, uint64_t(cap) * uint64_t(w), k, k > 1 ? kFrameRowBlockSh : 0, w, h,
                                out, uint64_t(w), root.gs);
    VRT_HIP(ctx, hipGetLastError());
  } else {
    for (int32_t j = 0; j < k; ++j) {  // each band's blocks into their frame rows
      BandCopy bc[2];
      const int nc = band_copies(w, h, k, frame_block(k), j, 4, bc);
      for (int c = 0; c < nc; ++c)
        VRT_HIP(ctx, hipMemcpy2DAsync(reinterpret_cast<char*>(out) + bc[c].dst_off, bc[c].dst_pitch,
                                      reinterpret_cast<const char*>(src[j]) + bc[c].src_off, bc[c].src_pitch,
                                      bc[c].width, bc[c].rows, hipMemcpyDeviceToDevice, root.gs));
    }
  }
  if (!ctx->distinct)
    for (int32_t j = 0; j < k; ++j) {  // same physical device: the bands were read here
      VRT_HIP(ctx, hipEventRecord(ctx->sh[j].ev_band_read[slot], root.gs));
      ctx->sh[j].band_read_valid[slot] = true;
    }
  VRT_HIP(ctx, hipEventRecord(ctx->ev_gathered, root.gs));
  *d_frame = out;
  return VRT_OK;
}

}  // namespace vrt

using namespace vrt;

extern "C" {

int vrt_render(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, float* out_rgba, vrt_hit* out_hit,
               vrt_stats* stats) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_render_args(ctx, cam, p);
  if (st != VRT_OK) return st;
  if (!out_rgba) return fail(ctx, VRT_ERR_INVALID, "null output");
  DeviceGuard guard;
  const int32_t k = int32_t(ctx->sh.size());
  const size_t pixels = size_t(band_cap(cam->height, k)) * size_t(cam->width);
  for (Shard& s : ctx->sh) {
    if (pixels <= s.out_pixels) continue;
    VRT_HIP(ctx, hipSetDevice(s.device));
    VRT_HIP(ctx, hipDeviceSynchronize());
    if (s.d_out) (void)hipFree(s.d_out);
    if (s.d_hit) (void)hipFree(s.d_hit);
    s.d_out = nullptr;
    s.d_hit = nullptr;
    s.out_pixels = 0;
    if (hipMalloc(&s.d_out, pixels * sizeof(float4)) != hipSuccess ||
        hipMalloc(&s.d_hit, pixels * sizeof(vrt_hit)) != hipSuccess)
      return fail(ctx, VRT_ERR_OOM, "hipMalloc frame buffers");
    s.out_pixels = pixels;
  }
  const size_t frame_px = size_t(cam->width) * size_t(cam->height);
  const size_t fbytes = frame_px * sizeof(float4), hbytes = out_hit ? frame_px * sizeof(vrt_hit) : 0;
  if ((st = ensure_stage(ctx, fbytes + hbytes)) != VRT_OK) return st;
  const bool counting = stats && (stats->request & VRT_STATS_COUNTERS);
  const int g = int(ctx->fk % kLanes);
  FrameMode mode;  // the float band (+ hit records) of a frame that runs alone
  mode.hits = out_hit != nullptr;
  mode.counting = counting;
  mode.timing = stats != nullptr;
  if ((st = launch_frame(ctx, cam, p, 1.0f, mode)) != VRT_OK) return st;
  std::vector<const void*> bands, hbands;
  for (Shard& s : ctx->sh) {
    bands.push_back(s.d_out);
    hbands.push_back(s.d_hit);
  }
  if ((st = stage_bands(ctx, g, cam->width, cam->height, bands.data(), sizeof(float4), 0)) != VRT_OK) return st;
  if (out_hit && (st = stage_bands(ctx, g, cam->width, cam->height, hbands.data(), sizeof(vrt_hit), fbytes)) != VRT_OK)
    return st;
  if ((st = finish_frame(ctx, stats, counting)) != VRT_OK) return st;
  std::memcpy(out_rgba, ctx->h_stage.p, fbytes);
  if (out_hit) std::memcpy(out_hit, ctx->h_stage.p + fbytes, hbytes);
  ctx->err.clear();
  return VRT_OK;
}

int vrt_render_frame(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, float alpha, uint8_t* out_rgba8,
                     vrt_stats* stats) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_render_args(ctx, cam, p);
  if (st != VRT_OK) return st;
  if (!out_rgba8) return fail(ctx, VRT_ERR_INVALID, "null output");
  DeviceGuard guard;
  if ((st = ensure_history(ctx, cam->width, cam->height)) != VRT_OK) return st;
  const size_t bytes = size_t(cam->width) * size_t(cam->height) * 4;
  if ((st = ensure_stage(ctx, bytes)) != VRT_OK) return st;
  const bool counting = stats && (stats->request & VRT_STATS_COUNTERS);
  const int g = int(ctx->fk % kLanes), slot = int(ctx->fk % kRing);
  FrameMode mode;  // the temporal path, a frame that runs alone
  mode.rgba8 = true;
  mode.counting = counting;
  mode.timing = stats != nullptr;
  if ((st = launch_frame(ctx, cam, p, alpha, mode)) != VRT_OK) return st;
  std::vector<const void*> bands;
  for (Shard& s : ctx->sh) bands.push_back(s.d_ring[slot]);
  ctx->fk++;
  if ((st = stage_bands(ctx, g, cam->width, cam->height, bands.data(), 4, 0)) != VRT_OK) return st;
  if ((st = finish_frame(ctx, stats, counting)) != VRT_OK) return st;
  std::memcpy(out_rgba8, ctx->h_stage.p, bytes);
  ctx->err.clear();
  return VRT_OK;
}

int vrt_render_frame_device(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, float alpha,
                            void* hip_stream, const uint32_t** d_frame, vrt_stats* stats) {
  if (!ctx) return VRT_ERR_INVALID;
  int st = check_render_args(ctx, cam, p);
  if (st != VRT_OK) return st;
  if (!d_frame) return fail(ctx, VRT_ERR_INVALID, "null frame pointer");
  DeviceGuard guard;
  if ((st = ensure_history(ctx, cam->width, cam->height)) != VRT_OK) return st;
  const bool counting = stats && (stats->request & VRT_STATS_COUNTERS);
  const int32_t k = int32_t(ctx->sh.size()), w = cam->width, h = cam->height;
  Shard& root = ctx->sh[0];
  hipStream_t cs = static_cast<hipStream_t>(hip_stream);
  const uint64_t f = ctx->fk;
  const int slot = int(f % kRing), g = int(f % kLanes);
  FrameMode mode;  // the temporal path, a frame that overlaps its neighbours on the other lanes
  mode.rgba8 = true;
  mode.counting = counting;
  mode.timing = stats != nullptr;
  mode.overlap = true;
  VRT_HIP(ctx, hipSetDevice(root.device));
  if (!cs) {
    // no caller stream (ABI v9): the caller consumes each frame on the stream that produced it
    // (vrt_frame_stream), which renders the frame that next reuses its buffer, kRing frames later,
    // after that consumption: no ordering packet between streams. One launch per band (so that one
    // stream holds the whole frame), and the host stays at most kRing frames ahead.
    if (ctx->slot_valid[slot] && hipEventQuery(ctx->ev_slot[slot]) != hipSuccess)
      VRT_HIP(ctx, hipEventSynchronize(ctx->ev_slot[slot]));
    // a caller that switched from its own stream to NULL: the frame this slot held may still be
    // read there (its consumption was enqueued before call f - kRing + 1)
    if (f >= kRing) {
      const int rs = int((f - kRing + 1) % kRing);
      if (ctx->consumed_valid[rs]) {
        if (hipEventQuery(ctx->ev_consumed[rs]) != hipSuccess) VRT_HIP(ctx, hipEventSynchronize(ctx->ev_consumed[rs]));
        ctx->consumed_valid[rs] = false;
      }
    }
    mode.one_part = true;
    if ((st = launch_frame(ctx, cam, p, alpha, mode)) != VRT_OK) return st;
    if (k == 1 && !ctx->coll1) {
      ctx->frame_stream = root.ls[g][0];
      *d_frame = root.d_ring[slot];
    } else {
      if ((st = gather_frame(ctx, w, h, slot, g, d_frame)) != VRT_OK) return st;
      ctx->frame_stream = root.gs;
    }
    VRT_HIP(ctx, hipSetDevice(root.device));
    VRT_HIP(ctx, hipEventRecord(ctx->ev_slot[slot], ctx->frame_stream));
    ctx->slot_valid[slot] = true;
    ctx->fk++;
    if (stats && (st = finish_frame(ctx, stats, counting)) != VRT_OK) return st;
    ctx->err.clear();
    return VRT_OK;
  }
  // E_f: whatever the caller enqueued on its stream so far (its consumption of frames <= f - 1)
  VRT_HIP(ctx, hipEventRecord(ctx->ev_consumed[slot], cs));
  ctx->consumed_valid[slot] = true;
  // Frame f overwrites the buffer handed out at frame f - kRing, which the caller's work before
  // call f - kRing + 1 consumed: E_{f-kRing+1}. The host waits for it when it is not done yet
  // (the caller's stream is more than kRing - 1 frames behind): a swapchain's back-pressure, with
  // no ordering packet on the GPU. (Waiting for it on the lane's stream cost 0.016 ms per C3 frame:
  // the cross-queue wait packets stalled the lanes; profiles/r03_s14; the one-off script is in git history.)
  if (f >= kRing) {
    const int rs = int((f - kRing + 1) % kRing);
    if (ctx->consumed_valid[rs] && hipEventQuery(ctx->ev_consumed[rs]) != hipSuccess)
      VRT_HIP(ctx, hipEventSynchronize(ctx->ev_consumed[rs]));
  }
  if (k == 1 && !ctx->coll1) {
    // one device: the frame is rendered straight into the ring slot handed to the caller; up to
    // kLanes frames in flight (u_Alpha = 1: independent frames)
    if ((st = launch_frame(ctx, cam, p, alpha, mode)) != VRT_OK) return st;
    for (int q = 0; q < root.lane_parts[g]; ++q) VRT_HIP(ctx, hipStreamWaitEvent(cs, root.ev_done[g][q], 0));
    *d_frame = root.d_ring[slot];
  } else {
    if ((st = launch_frame(ctx, cam, p, alpha, mode)) != VRT_OK) return st;
    if ((st = gather_frame(ctx, w, h, slot, g, d_frame)) != VRT_OK) return st;
    VRT_HIP(ctx, hipSetDevice(root.device));
    VRT_HIP(ctx, hipStreamWaitEvent(cs, ctx->ev_gathered, 0));
  }
  ctx->fk++;
  if (stats && (st = finish_frame(ctx, stats, counting)) != VRT_OK) return st;
  ctx->err.clear();
  return VRT_OK;
}

void* vrt_frame_stream(const vrt_ctx* ctx) { return ctx ? static_cast<void*>(ctx->frame_stream) : nullptr; }

int vrt_history_reset(vrt_ctx* ctx) {
  if (!ctx) return VRT_ERR_INVALID;
  // key F (main.cpp:417-421): std::swap(lastFrameBuffer, rayTraceFrameBuffer) — the next frame
  // filters against the last ray-traced frame. No buffer changes hands: the next frame reads its
  // history from the last frame's raw band (its filtered band when u_Alpha was 1, where the two
  // are equal), so a device-output frame the caller still holds stays untouched.
  ctx->reset_pending = ctx->fk > 0;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_comm_unique_id(uint8_t* out, int32_t bytes) {
  static_assert(sizeof(ncclUniqueId) == VRT_COMM_ID_BYTES, "RCCL unique id size");
  if (!out || bytes < VRT_COMM_ID_BYTES) return VRT_ERR_INVALID;
  ncclUniqueId id;
  if (ncclGetUniqueId(&id) != ncclSuccess) return VRT_ERR_DEVICE;
  std::memcpy(out, &id, sizeof(id));
  return VRT_COMM_ID_BYTES;
}

int vrt_comm_join(vrt_ctx* ctx, const uint8_t* ids, int32_t count, int32_t nranks, int32_t rank) {
  if (!ctx) return VRT_ERR_INVALID;
  if (ctx->sh.size() != 1) return fail(ctx, VRT_ERR_INVALID, "vrt_comm_join: a one-device context per rank");
  if (!ids || count < 1 || count > 16 || nranks < 1 || rank < 0 || rank >= nranks)
    return fail(ctx, VRT_ERR_INVALID, "vrt_comm_join: 1..16 ids, 0 <= rank < nranks");
  if (!ctx->rank_comms.empty()) return fail(ctx, VRT_ERR_INVALID, "vrt_comm_join: already joined");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  for (int32_t i = 0; i < count; ++i) {  // every rank in the same order: each init waits for all ranks
    ncclUniqueId id;
    std::memcpy(&id, ids + size_t(i) * VRT_COMM_ID_BYTES, sizeof(id));
    ncclComm_t cm = nullptr;
    const ncclResult_t r = ncclCommInitRank(&cm, nranks, id, rank);
    if (r != ncclSuccess) {
      for (ncclComm_t c2 : ctx->rank_comms) (void)ncclCommDestroy(c2);
      ctx->rank_comms.clear();
      return nccl_fail(ctx, r, "ncclCommInitRank");
    }
    ctx->rank_comms.push_back(cm);
  }
  ctx->rank_nranks = nranks;
  ctx->rank_id = rank;
  ctx->err.clear();
  return VRT_OK;
}

int vrt_gather_band_async(vrt_ctx* ctx, int32_t comm, const void* d_band, uint64_t bytes, void* d_gathered,
                          void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (comm < 0 || size_t(comm) >= ctx->rank_comms.size())
    return fail(ctx, VRT_ERR_INVALID, "vrt_gather_band_async: no such communicator (vrt_comm_join)");
  if (!d_band || (ctx->rank_id == 0 && !d_gathered))
    return fail(ctx, VRT_ERR_INVALID, "vrt_gather_band_async: null band or (root) gather buffer");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  VRT_NCCL(ctx, ncclGather(d_band, ctx->rank_id == 0 ? d_gathered : nullptr, size_t(bytes), ncclUint8, 0,
                           ctx->rank_comms[size_t(comm)], static_cast<hipStream_t>(hip_stream)));
  return VRT_OK;
}

int vrt_pack_rgb8_async(vrt_ctx* ctx, const uint32_t* d_rgba8, uint64_t pixels, uint8_t* d_rgb8, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!d_rgba8 || !d_rgb8 || pixels % 4 != 0 || (reinterpret_cast<uintptr_t>(d_rgba8) & 15u) ||
      (reinterpret_cast<uintptr_t>(d_rgb8) & 3u))
    return fail(ctx, VRT_ERR_INVALID, "vrt_pack_rgb8_async: pixels % 4, 16-byte RGBA8 and 4-byte RGB8 alignment");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  vrt::launch_pack_rgb8(d_rgba8, pixels, d_rgb8, static_cast<hipStream_t>(hip_stream));
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

int vrt_assemble_blocks_rgb8_async(vrt_ctx* ctx, const uint8_t* d_bands, int32_t k, int32_t band_rows_cap,
                                   int32_t width, int32_t height, int32_t row_block, uint32_t* d_frame,
                                   int64_t frame_pitch, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  int32_t sh = 0;
  while (sh < 7 && (1 << sh) != row_block) ++sh;
  if (sh == 7) return fail(ctx, VRT_ERR_INVALID, "row_block must be a power of two in [1, 64]");
  if (!d_bands || !d_frame || k < 1 || width < 4 || width % 4 || height < 1 || frame_pitch < width ||
      frame_pitch % 4 || (reinterpret_cast<uintptr_t>(d_frame) & 15u) || (reinterpret_cast<uintptr_t>(d_bands) & 3u))
    return fail(ctx, VRT_ERR_INVALID,
                "vrt_assemble_blocks_rgb8_async: width and pitch multiples of 4, 16-byte frame, 4-byte bands");
  if (largest_band(height, k, row_block) > band_rows_cap)
    return fail(ctx, VRT_ERR_INVALID, "vrt_assemble_blocks_rgb8_async: band_rows_cap below the largest band");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  vrt::launch_assemble_blocks_rgb8(d_bands, uint64_t(band_rows_cap) * uint64_t(width), k, sh, width, height, d_frame,
                                   uint64_t(frame_pitch), static_cast<hipStream_t>(hip_stream));
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

int vrt_assemble_blocks_async(vrt_ctx* ctx, const uint32_t* d_bands, int32_t k, int32_t band_rows_cap,
                              int32_t width, int32_t height, int32_t row_block, uint32_t* d_frame,
                              int64_t frame_pitch, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  int32_t sh = 0;
  while (sh < 7 && (1 << sh) != row_block) ++sh;
  if (sh == 7) return fail(ctx, VRT_ERR_INVALID, "row_block must be a power of two in [1, 64]");
  if (!d_bands || !d_frame || k < 1 || width < 1 || height < 1 || frame_pitch < width)
    return fail(ctx, VRT_ERR_INVALID, "vrt_assemble_blocks_async: bad buffers or sizes");
  if (largest_band(height, k, row_block) > band_rows_cap)   // every band must fit its slice
    return fail(ctx, VRT_ERR_INVALID, "vrt_assemble_blocks_async: band_rows_cap below the largest band");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(ctx->sh[0].device));
  vrt::launch_assemble_blocks(d_bands, uint64_t(band_rows_cap) * uint64_t(width), k, sh, width, height, d_frame,
                              uint64_t(frame_pitch), static_cast<hipStream_t>(hip_stream));
  VRT_HIP(ctx, hipGetLastError());
  return VRT_OK;
}

}  // extern "C"
