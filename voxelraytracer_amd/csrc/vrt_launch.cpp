// vrt_launch.cpp — one band launch: the kernel argument block of a camera, params and band (make_args), the
// tile-order and deferred-list slots of a shard's pool, and launch(), which decides per launch between the
// deferred exact pass, the heavy-first tile order and dispatch order (vrt_context.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "vrt_context.h"

namespace vrt {

// KArgs::defer: two sets of segment counters, then the list: a pixel per word, 8 segments of
// ceil(tiles / 8) tiles' pixels each. Allocated per tile-order slot at its first deferred launch,
// sized for that band (a 1080p band: 8.3 MB; until r03 every slot was sized for 65 536 tiles up
// front, 537 MB per device).
// tiles of the largest segment: a column block of the band (tile columns tx * 8 / tiles_x)
static uint32_t defer_seg_tiles(uint32_t tiles, uint32_t tiles_x) {
  return (tiles_x + vrt::kOrdClasses - 1u) / vrt::kOrdClasses * (tiles / tiles_x);
}
static size_t defer_words(uint32_t tiles, uint32_t tiles_x) {
  return vrt::kDeferHdr + size_t(vrt::kOrdClasses) * defer_seg_tiles(tiles, tiles_x) * vrt::kWgThreads;
}

// KArgs::ostride: bytes from one octant's packed (N+1)^3 u16 volume to the next (0: a single volume)
uint32_t octant_stride(const Shard& s) {
  return s.octants == 8 ? uint32_t(uint64_t(s.n + 1) * (s.n + 1) * (s.n + 1) * sizeof(uint16_t)) : 0u;
}

vrt::KArgs make_args(const vrt_ctx* ctx, const Shard& s, const vrt_camera* cam, const vrt_params* p,
                     int32_t row0, int32_t rows, int32_t row_step) {
  vrt::KArgs a;
  std::memcpy(a.inv_pv, cam->inv_pv, sizeof(a.inv_pv));
  std::memcpy(a.sun, p->sun_dir, sizeof(a.sun));
  a.sky_sy = std::fmax(p->sun_dir[1], 0.0f);  // GLSL max(x, 0) with fmaxf's NaN rule, as gmax
  fill_sun(a, p->sun_dir);
  a.time = p->time;
  a.ray_noise = p->ray_noise;
  a.refl_noise = p->reflection_noise;
  a.refr_noise = p->refraction_noise;
  a.max_len = p->max_ray_length;
  a.n = s.n;
  a.fn = float(s.n);
  a.width = cam->width;
  a.height = cam->height;
  a.rcp_w = 1.0f / float(cam->width);
  a.rcp_h = 1.0f / float(cam->height);
  a.row0 = row0;
  a.rows = rows;
  a.row_step = row_step;
  a.row_blk_sh = 0;
  a.pitch = cam->width;
  a.ostride = octant_stride(s);
  vrt::sun_consts(a);  // (after sun_n and ostride)
  a.max_refl = p->max_reflections;
  a.max_transp = p->max_transparencies;
  a.textured = p->color_only ? 0 : 1;
  a.atlas_size = p->color_only ? 1 : p->atlas_size;
  a.atlas_tex_size = p->atlas_texture_size;
  a.atlas = s.d_atlas;
  a.alpha = 1.0f;
  vrt::setup_consts(a);        // (after width, height, fn and max_len)
  a.vdiv_ok = 0;
  vrt::cert_launch_consts(a);  // all clear; set per launch (launch)
  // of this camera; launch() clears it when a later frame of a batch fails the test
  a.vdiv_ok = vrt::vertex_div_ranges_ok(a.inv_pv) ? 1u : 0u;
  a.prev = nullptr;
  a.cur = nullptr;
  a.raw = nullptr;
  // automatic mode: certified pixels unless glass dominates the volume, where certified bounce
  // trees (automatic: exactly those volumes) settle the glass pixels instead
  const bool trees = ctx->tree_req == 2 || (ctx->tree_req == 1 && !s.cert_auto);
  a.cert = s.octants != 8 || ctx->cert_req < 0 ? 0 : (ctx->cert_req > 0 || s.cert_auto || trees ? 2 : 1);
  a.tree = a.cert == 2 && p->color_only && trees ? 1 : 0;
  a.tiles_x = uint32_t((a.width + vrt::kTileW - 1) / vrt::kTileW);
  a.tiles = a.tiles_x * uint32_t((a.rows + vrt::kTileH - 1) / vrt::kTileH);
  a.order = nullptr;
  a.ord_r = a.ord_w = a.ctr_r = a.ctr_w = a.ctr_z = a.ord_q = 0;
  a.defer = nullptr;
  a.defer_e = a.defer_seg = 0;
  a.exact_fat = 0;
  a.exact_grid = 0;
  a.batches_out = nullptr;
  a.nframes = 1;
  a.frame_tiles = a.tiles;
  std::memset(a.fb, 0, sizeof(a.fb));
  return a;
}

// The tile-order slot of this launch's band and stream, from the shard's pool (no allocation, no
// host sync in the steady state). A slot stays with its (band, stream): launches on one stream are
// ordered, so no marker is needed per launch while the pool has room (a frame loop uses one slot per
// lane). Reassigning the least recently used slot to another band or stream (more pairs than
// kOrderSlots) must first wait for the old stream's last launch with the slot, and that stream may
// already have been destroyed by its owner, so nothing can be recorded on it then: once half the
// pool has been assigned, every launch with a slot records the slot's ev_last after it
// (slot_launched), and eviction waits for that event; a slot evicted before any such record (the
// pool filled in one burst) falls back to a device synchronisation. Then the slot is zeroed on this
// stream (no heavy tiles yet). Not while the stream is being captured into a graph (a replayed node
// would reuse one list / counter set): dispatch order then.
static OrderSlot* acquire_slot(Shard& s, const vrt::KArgs& a, hipStream_t st) {
  if (a.tiles == 0 || a.tiles > kOrderMaxTiles) return nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return nullptr;
  OrderSlot* slot = nullptr;
  for (auto& o : s.order)
    if (o.used && o.width == a.width && o.rows == a.rows && o.row0 == a.row0 && o.row_step == a.row_step &&
        o.row_blk_sh == a.row_blk_sh && o.nframes == a.nframes && o.stream == st)
      slot = &o;
  if (!slot) {
    slot = &s.order[0];
    for (auto& o : s.order)
      if (!o.used || (slot->used && o.tick < slot->tick)) slot = &o;
    if (slot->used && slot->stream != st) {
      const hipError_t e = slot->ev_last_valid ? hipEventSynchronize(slot->ev_last) : hipDeviceSynchronize();
      if (e != hipSuccess) return nullptr;
    }
    slot->ev_last_valid = false;
    ++s.order_assigned;
    // zero the list counters, the wave counters and both rank sets (no heavy tiles yet)
    if (hipMemsetAsync(slot->d, 0, (vrt::kOrdHdr + size_t(3) * a.tiles) * sizeof(uint32_t), st) != hipSuccess)
      return nullptr;
    slot->width = a.width;
    slot->rows = a.rows;
    slot->row0 = a.row0;
    slot->row_step = a.row_step;
    slot->row_blk_sh = a.row_blk_sh;
    slot->nframes = a.nframes;
    slot->stream = st;
    slot->epoch = 0;
    slot->last_defer = false;
    slot->used = true;
  }
  slot->tick = ++s.order_tick;
  return slot;
}

// After a launch with slot `o` on st: under pool pressure, mark its end for a later eviction.
static void slot_launched(Shard& s, OrderSlot* o, hipStream_t st) {
  if (!o || s.order_assigned * 2u < uint32_t(kOrderSlots)) return;
  if (!o->ev_last && hipEventCreateWithFlags(&o->ev_last, hipEventDisableTiming) != hipSuccess) {
    o->ev_last = nullptr;
    return;
  }
  o->ev_last_valid = hipEventRecord(o->ev_last, st) == hipSuccess;
}

// A frame that runs alone (synchronous calls) with the deferred exact pass, as one launch with the
// exact pass's short-band instance: where the in-lane alternative's long waves are the frame
// (glass-heavy volumes: every lane holds its bounce tree) or the certified pass is long enough to
// carry the exact pass's ~50 us tail (>= 8 rounds of resident waves); frames of at least two rounds
// (the deferral's own bound, launch_state_begin) within one list slot. Synchronous frames, device
// timestamps: C1 0.330 -> 0.252 ms, C4 0.247 -> 0.212; C3 0.101 -> 0.103 and C2 0.129 -> 0.146
// stay in lane, as two interleaved parts (profiles/r06_s12).
bool lone_defers(const vrt_ctx* ctx, const Shard& s, const vrt::KArgs& a) {
  const uint32_t waves = a.tiles * uint32_t(vrt::kWgWaves);
  return ctx->exact_pass > 0 && a.cert == 2 && !a.textured && a.rows < 8192 && a.tiles <= kOrderMaxTiles &&
         waves >= 2u * s.wave_slots && (!s.cert_auto || waves >= 8u * s.wave_slots);
}

// Per-launch state of a stats-free launch from its slot: the deferred exact pass's mask buffer
// (certified colour-only launches, vrt_set_exact_pass), else the heavy-first tile order.
// allow_defer: false for frames that run alone (synchronous calls): there the exact pass's
// latency after the certified pass is the frame's (C3 0.198 vs 0.076 ms per synchronous frame),
// while frames in flight hide it. The deferral also needs a launch of at least two rounds of the
// certified pass's resident waves: on smaller bands the exact pass's latency (its longest waves
// are the glass pixels' bounce stacks) follows a short certified pass on the same stream and
// bounds the band's frame rate (C3's band at k = 4 / 8 GPUs: 0.025 / 0.0235 ms per frame deferred,
// 0.0155 / 0.0114 in-lane; the whole frame: 0.0445 deferred, 0.060 in-lane; C4's band at k = 8,
// 16 200 waves: 0.0281 deferred, 0.0297 in-lane; profiles/r03_s18, r03_s19).
static OrderSlot* launch_state_begin(const vrt_ctx* ctx, Shard& s, vrt::KArgs& a, hipStream_t st, LaunchMode mode) {
  const bool allow_defer = mode.allow_defer || mode.lone, lone = mode.lone;
  // (the deferred list packs a pixel as frame | band row | column in 3 | 13 | 16 bits)
  const bool defer = allow_defer && ctx->exact_pass > 0 && a.cert == 2 && a.rows < 8192 &&
                     (ctx->exact_pass == 2 || a.tiles * uint32_t(vrt::kWgWaves) >= 2u * s.wave_slots);
  // the tile order only where it pays: glass in the volume (without it the order gains nothing:
  // C2 ±0, C4 +5 %, profiles/r02_s14_tileorder) and certified pixels (glass-heavy volumes, where
  // every tile is heavy, keep dispatch order: C1 +3.4 %)
  // Nor for launches below one dispatch round of waves (kOrdMinRounds): all of their tiles are
  // resident at once, so an order only costs its list reads and bookkeeping (C3's 8-way bands
  // in flight: rank 7 0.0078 -> 0.0072, rank 6 0.0127 -> 0.0105 ms per frame, profiles/r05_s14)
  const bool order = !defer && ctx->tile_order != 0 && !a.textured && a.cert == 2 && s.has_glass &&
                     (ctx->tile_order == 2 ||
                      a.tiles * uint32_t(vrt::kWgWaves) >= vrt::kOrdMinRounds * s.wave_slots);
  if (!defer && !order) return nullptr;
  OrderSlot* slot = acquire_slot(s, a, st);
  if (!slot) return nullptr;
  if (defer) {  // both counter sets zeroed whenever the slot's previous launch was not one
    const size_t need = defer_words(a.tiles, a.tiles_x);
    if (slot->defer_cap < need) {  // first deferred launch of this band on the slot (or a larger band)
      // earlier launches with the slot run on st (its stream) and may still read the old list
      if (slot->defer && (hipStreamSynchronize(st) != hipSuccess || hipFree(slot->defer) != hipSuccess)) return slot;
      slot->defer = nullptr;
      slot->defer_cap = 0;
      if (hipMalloc(&slot->defer, need * sizeof(uint32_t)) != hipSuccess) {
        slot->defer = nullptr;
        return slot;  // no list: the launch keeps the exact path in lane
      }
      slot->defer_cap = need;
      slot->last_defer = false;
    }
    uint32_t* d = slot->defer;
    if (!slot->last_defer) {
      if (hipMemsetAsync(d, 0, vrt::kDeferHdr * sizeof(uint32_t), st) != hipSuccess) return slot;
      slot->defer_epoch = 0;
    }
    a.defer = d;
    a.defer_e = uint32_t(slot->defer_epoch & 1u);
    a.defer_seg = defer_seg_tiles(a.tiles, a.tiles_x) * uint32_t(vrt::kWgThreads);
    // bands of under 4 rounds: the exact pass's latency follows a short certified pass
    a.exact_fat = !a.textured && (lone || a.tiles * uint32_t(vrt::kWgWaves) < 4u * s.wave_slots) ? 1 : 0;
    if (!a.exact_fat) {
      const uint32_t div = a.textured ? vrt::kDeferGridDiv : vrt::kDeferGridDivColor;  // launch_render's
      // the grid from an earlier frame's batch count on this slot (frames in flight: a few frames
      // old) plus a margin; a larger frame loops its workgroups over the rest. Idle workgroups
      // are not free: each waits for a register and LDS slot among the next frames' waves. Not for
      // short bands, whose frame time is this pass's span (C4 8-way band 0.0196 -> 0.0200 ms with
      // it, profiles/r04_s26)
      if (!slot->h_batches) {
        void* h = nullptr;
        if (hipHostMalloc(&h, sizeof(uint32_t), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) {
          slot->h_batches = static_cast<uint32_t*>(h);
          *slot->h_batches = ~0u;
          void* d = nullptr;
          if (hipHostGetDevicePointer(&d, h, 0) == hipSuccess) slot->d_batches = static_cast<uint32_t*>(d);
        }
      }
      if (slot->d_batches) {
        const uint32_t full = std::max(64u, a.tiles * uint32_t(vrt::kWgWaves) / div);
        const uint32_t prev = *static_cast<volatile uint32_t*>(slot->h_batches);
        a.batches_out = slot->d_batches;
        if (prev != ~0u) a.exact_grid = std::min(full, std::max(64u, prev + prev / 4u + 64u));
      }
    }
    slot->defer_epoch++;
    slot->last_defer = true;
    return slot;
  }
  slot->last_defer = false;
  a.order = slot->d;
  a.ord_r = uint32_t(slot->epoch & 1u);
  a.ord_w = a.ord_r ^ 1u;
  a.ctr_r = uint32_t(slot->epoch % 3u);
  a.ctr_w = (a.ctr_r + 1u) % 3u;
  a.ctr_z = (a.ctr_r + 2u) % 3u;
  a.ord_q = vrt::ord_q_for(a.tiles);
  slot->epoch++;
  return slot;
}

// One band launch on `st` (heavy-first tile order for uncounted launches), then, when counting,
// the fold of the counter replicas into `cnt` (accumulating). ev_begin / ev_end: optional device
// timestamps of the kernel's start and end. a.vdiv_ok: frame 0's, from make_args.
void launch(const vrt_ctx* ctx, Shard& s, vrt::KArgs a, float4* out, vrt_hit* hit, unsigned long long* cnt,
            hipStream_t st, hipEvent_t ev_begin, hipEvent_t ev_end, LaunchMode mode) {
  const bool stats = hit || cnt;
  for (int f = 1; f < a.nframes; ++f)
    if (!vertex_div_ranges_ok(a.fb[f - 1].inv_pv)) a.vdiv_ok = 0u;
  vrt::cert_launch_consts(a);
#ifdef VRT_SETUP_MASK  // make variant NAME=m<bits> DEFS=-DVRT_SETUP_MASK=<bits>: only these flags (per-flag A/B; 0: every fallback)
#ifndef VRT_DIAGNOSTIC_BUILD
#error "VRT_SETUP_MASK is a diagnostic build: use make variant"
#endif
  a.setup &= uint32_t(VRT_SETUP_MASK);
#endif
  OrderSlot* slot = stats ? nullptr : launch_state_begin(ctx, s, a, st, mode);
  vrt::launch_render(a, stats, s.d_vox_pad, out, hit, cnt ? s.d_cnt_rep : nullptr, st, ev_begin, ev_end);
  slot_launched(s, slot, st);
  if (cnt) vrt::launch_reduce_counters(s.d_cnt_rep, cnt, st);
}

// The next launch's timestamp events (vrt_set_launch_timing), or none when off / all in use
void launch_timing_events(vrt_ctx* ctx, hipEvent_t& begin, hipEvent_t& end) {
  begin = end = nullptr;
  if (ctx->lt_used + 2 > ctx->lt_ev.size()) return;
  begin = ctx->lt_ev[ctx->lt_used++];
  end = ctx->lt_ev[ctx->lt_used++];
}

}  // namespace vrt
