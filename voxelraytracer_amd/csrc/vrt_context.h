// vrt_context.h — the C-ABI context of include/vrt.h around the kernels of vrt_render.hip: its types,
// constants and the declarations its files share (file map: DESIGN.md §1). Not installed.
//
// A context spans the devices of its mask. Every device holds a "shard": a
// replica of the volume in the kernel's packed layout, kLanes lanes of context-owned streams, its
// row band's history / ray-trace / float buffers, counters and the tile-order pool. Whole-frame
// entry points split the frame into cyclic row bands (device j renders rows j, j+k, ...; sky and
// geometry rows balance across devices). Frame f renders on lane f % kLanes: device-output frames
// that do not read their history (u_Alpha = 1) are one launch per band and up to kLanes of them are
// in flight, the next frames' waves filling the slots one frame's longest waves hold; frames that
// run alone or read their history are two interleaved row parts, whose launches overlap each
// other's tails (DESIGN.md §6 "Tail hiding", §8 "Frames in flight"). The reference's single GL
// draw (main.cpp:323-361) becomes k (or 2k) concurrent launches.
// The only exchange is the output: synchronous host outputs are written by each device's DMA
// engine straight into its rows of a pinned staging frame (k links in parallel, no device hop);
// the device-output frame is gathered to the first device with ncclGather over xGMI
// (rccl.h:745). The volume reaches the other devices by ncclBroadcast from the first one.
#ifndef VRT_CONTEXT_H
#define VRT_CONTEXT_H

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdint>
#include <string>
#include <vector>

#include "vrt.h"
#include "vrt_bands.h"
#include "vrt_internal.h"

// context-private: nothing below is exported from the library
#pragma GCC visibility push(hidden)

namespace vrt {

constexpr int kParts = 2;              // interleaved row parts of a frame that runs alone
// Whole frames rotate over kLanes lanes: frame f renders on lane f % kLanes (kParts streams and
// timing events of its own) into history ring slot f % kRing. At u_Alpha = 1 a frame does not read
// its history, so consecutive device-output frames are independent and up to kLanes of them are in
// flight: the light waves of the next frames fill the wave slots one frame's exact-path waves hold
// (C3 0.0618 -> 0.0599 ms per frame on one GPU, C3's band at k = 8 GPUs 0.0416 -> 0.0112 ms;
// profiles/r03_pipe). Such frames are one launch (a second part
// only adds launch overhead once other frames fill the tail); frames that run alone (synchronous
// calls) or read their history (u_Alpha != 1: part q of frame f waits for part q of frame f - 1)
// are kParts interleaved parts, whose launches overlap each other's tails.
constexpr int kLanes = 4;
constexpr int kOrderSlots = 16;        // tile-order buffers per device (band geometry x stream)
constexpr uint32_t kOrderMaxTiles = 1u << 17;  // launches up to 131072 16x8 tiles (e.g. 7 frames of a 7-way 4K band)
constexpr size_t kOrderSlotWords = vrt::kOrdHdr + 5u * size_t(kOrderMaxTiles) + 2u * vrt::kOrdClasses;  // KArgs::order
// Filtered frames rotate through kRing buffers: frame f reads ring[(f-1) % kRing] (the temporal
// history) and writes ring[f % kRing]. A device-output frame (vrt_render_frame_device) is handed
// to the caller as its ring buffer and stays valid until the fourth later call, with no copy. Eight
// slots for four lanes: frame f overwrites the slot of frame f - 8, whose consumption the caller
// had enqueued well before frame f - 4 (frame f's predecessor on its lane) ends, so the wait for
// it costs nothing in the steady state (with four slots every frame waited for its lane
// predecessor's consumption through two command-processor hops: C3 0.0719 vs 0.0596 ms per frame).
constexpr int kRing = 8;
constexpr size_t kVstatWords = 8;  // Shard::d_vstats: 2 counts of an upload, 5 of an edit's box
static_assert(kRing % kLanes == 0, "a ring slot is always written from the same lane");

struct OrderSlot {
  int32_t width = 0, rows = 0, row0 = 0, row_step = 0, row_blk_sh = 0;
  int32_t nframes = 1;         // frames per launch (frame batches)
  hipStream_t stream = nullptr;
  uint32_t* d = nullptr;       // kOrderSlotWords words inside the shard's pool
  bool used = false;
  uint64_t epoch = 0, tick = 0;
  uint64_t defer_epoch = 0;    // deferred-pass launches since the slot's counters were zeroed
  bool last_defer = false;     // the slot's last launch was a deferred-pass launch
  uint32_t* defer = nullptr;   // the deferred pass's counters + list (lazily allocated)
  size_t defer_cap = 0;        // its words
  uint32_t* h_batches = nullptr;  // host-mapped: an earlier exact pass's batch count (~0u: none)
  uint32_t* d_batches = nullptr;  // its device address
  // end of the slot's last launch (recorded once the pool is under pressure, see acquire_slot):
  // evicting the slot waits for it instead of the whole device
  hipEvent_t ev_last = nullptr;
  bool ev_last_valid = false;
};

struct Shard {
  int device = 0;
  uint32_t wave_slots = 7168;  // resident waves of the certified pass: CUs x 4 SIMDs x 7
  // volume: canonical N^3, distance scratch, the kernel's packed octant volumes
  uint8_t* d_vox = nullptr;
  uint8_t* d_tmp = nullptr;
  uint16_t* d_vox_pad = nullptr;
  int32_t n = 0, octants = 0;
  bool cert_auto = true;   // automatic certified-pixel choice for the resident volume
  bool has_glass = true;   // the resident volume has glass (bounce stacks; tile order)
  unsigned long long* d_vstats = nullptr;  // glass and non-empty voxel counts (kVstatWords words)
  unsigned long long glass = 0, non_empty = 0;  // of the resident volume (an edit moves them by its box's)
  // counters
  unsigned long long* d_cnt = nullptr;      // VRT_CNT_COUNT totals of a synchronous render
  unsigned long long* d_cnt_rep = nullptr;  // kCntReplicas x VRT_CNT_COUNT, kept zeroed
  // whole-frame lanes: streams, and per lane the events of its last frame's launches
  hipStream_t ls[kLanes][kParts] = {};
  hipEvent_t ev_done[kLanes][kParts] = {};
  int lane_parts[kLanes] = {};       // launches of the lane's last frame (0: none)
  int slot_reader[kRing] = {};       // lane + 1 of the frame that read slot s as its history (0: none)
  hipStream_t gs = nullptr;          // gather / assembly / host-copy stream
  hipEvent_t ev_gs = nullptr;        // marker on gs (volume upload ordering, gather done)
  hipEvent_t ev_band_read[kRing] = {};  // gs has read ring slot s (device-output gather)
  bool band_read_valid[kRing] = {};
  // GPU time of each launch of the last synchronous frame: recorded when the kernel starts /
  // ends on the device
  hipEvent_t ev_kbeg[kParts] = {}, ev_kend[kParts] = {};
  bool timed[kParts] = {};
  // this device's row band of the whole-frame buffers (band_cap rows x width)
  uint32_t* d_ring[kRing] = {};      // filtered bands (history ring)
  uint32_t* d_rawbuf[kRing] = {};    // quantised ray-trace band of frame f (rayTrace FBO; key F)
  size_t hist_pixels = 0;
  float4* d_out = nullptr;     // vrt_render's float band
  vrt_hit* d_hit = nullptr;
  size_t out_pixels = 0;
  // textured mode's atlas (RGBA8 words)
  uint32_t* d_atlas = nullptr;
  int32_t atlas_size = 0;
  // heavy-first tile order, and the deferred exact pass's lists (same slots)
  uint32_t* d_order_pool = nullptr;
  OrderSlot order[kOrderSlots];
  uint64_t order_tick = 0;
  uint32_t order_assigned = 0;  // (band, stream) pairs assigned to slots so far
};

// A staging buffer a context owns and grows on demand: device memory, or (Pinned) portable pinned host
// memory that every device's DMA engine writes directly. Contents do not survive an alloc. The buffer's
// device is current whenever it is allocated or released (vrt_destroy makes it so before the context's
// buffers release themselves).
template <class T, bool Pinned = false>
struct Stage {
  T* p = nullptr;
  size_t cap = 0;  // elements
  Stage() = default;
  Stage(const Stage&) = delete;
  Stage& operator=(const Stage&) = delete;
  ~Stage() { release(); }
  void release() {
    if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  // n elements in place of the old ones; false, and empty, when the allocation fails
  bool alloc(size_t n) {
    release();
    void* q = nullptr;
    if ((Pinned ? hipHostMalloc(&q, n * sizeof(T), hipHostMallocPortable) : hipMalloc(&q, n * sizeof(T))) != hipSuccess)
      return false;
    p = static_cast<T*>(q);
    cap = n;
    return true;
  }
};
// A group of stagings that grow together, all or nothing: every buffer is released, then allocated at n
// elements; after a failure all of them are empty.
template <class... S>
bool stage_alloc_all(size_t n, S&... s) {
  (s.release(), ...);
  if ((s.alloc(n) && ...)) return true;
  (s.release(), ...);
  return false;
}

}  // namespace vrt

struct vrt_ctx {
  std::vector<vrt::Shard> sh;
  bool distinct = true;                 // devices pairwise distinct: RCCL communicators exist
  bool coll1 = false;                   // one device through the RCCL path (vrt_debug_collectives)
  std::vector<ncclComm_t> comms;
  int32_t layout_req = 0;               // vrt_set_skip_layout
  int32_t cert_req = 0;                 // vrt_set_certified
  int32_t tree_req = 1;                 // vrt_set_cert_trees
  int tile_order = 1;                   // vrt_set_tile_order: 0 off, 1 automatic, 2 always
  int32_t exact_pass = 1;               // vrt_set_exact_pass: 0 off, 1 automatic, 2 always
  // vrt_set_launch_timing: timing events for the async band launches' device start / end
  // timestamps (2 per launch, created up front), and how many are in use since the last read
  std::vector<hipEvent_t> lt_ev;
  size_t lt_used = 0;
  std::vector<uint8_t> atlas_host;      // bytes of the last atlas upload (a params pointer is
                                        // re-uploaded when its bytes differ, not by identity)
  int32_t hist_w = 0, hist_h = 0;       // image size of the resident whole-frame history
  uint64_t fk = 0;                      // frames rendered into the resident history
  bool raw_is_cur[vrt::kRing] = {};     // frame in slot s had u_Alpha = 1: its raw frame = ring[s]
  bool reset_pending = false;           // vrt_history_reset: the next frame's history is the raw frame
  uint32_t* d_gather = nullptr;         // first device: k x band_cap x width words (ncclGather)
  size_t hist_pixels_gather = 0;
  uint32_t* d_frames[vrt::kRing] = {};  // first device, k > 1: assembled frames
  // caller stream, device-output frames: E_f = ev_consumed[f % kRing], recorded at call f, marks
  // the caller's work enqueued before call f (its consumption of frames <= f - 1)
  hipEvent_t ev_consumed[vrt::kRing] = {};
  bool consumed_valid[vrt::kRing] = {};
  hipEvent_t ev_gathered = nullptr;     // first device: the last device-output frame is assembled
  // device-output frames with no caller stream (vrt_frame_stream): the stream that rendered (or
  // assembled) the last frame, and per ring slot the end of the frame rendered into it (host
  // back-pressure: at most kRing frames ahead)
  hipStream_t frame_stream = nullptr;
  hipEvent_t ev_slot[vrt::kRing] = {};
  bool slot_valid[vrt::kRing] = {};
  vrt::Stage<char, true> h_stage;       // pinned host staging of synchronous frames (k bands in), bytes
  // first device: staging of the synchronous ray queries (vrt_cast_rays, vrt_pick_pixels, vrt_trace_rays,
  // vrt_trace_pixels), records of 32 bytes each in and out (the input also holds pixel pairs); grows on demand
  vrt::Stage<vrt_ray> d_query_in;
  vrt::Stage<vrt_ray_hit> d_query_out;
  // first device: staging of the synchronous ID and depth pass (vrt_render_ids): records and depths,
  // grown to the largest frame. ids_pixels / ids_deferred: of the last such call (vrt_ids_deferred).
  // d_ids_count: one word, allocated with the staging: the certified ID kernel's exact-path pixels of a
  // synchronous call (zeroed on the main stream before the launch, copied back with the frame; the
  // capturable entry point never passes it). ids_cert_req: vrt_set_ids_certified
  vrt::Stage<vrt_pixel_id> d_ids_stage;
  vrt::Stage<float> d_depth_stage;
  vrt::Stage<uint32_t> d_ids_count;
  uint64_t ids_pixels = 0, ids_deferred = 0;
  int32_t ids_cert_req = 0;
  // first device: vrt_render_frame_reprojected's staging for frames of rp_w x rp_h (grown to the largest frame):
  // the raw frame, the depth, ping-pong filtered frames and noise-free ID buffers (rp_cur: the last call's),
  // the last call's forward matrix, and whether the next call has a history (rp_valid). Separate from
  // vrt_render_frame's ring. ev_rp_beg / ev_rp_end: device timestamps of a call's first and last launch
  vrt::Stage<uint32_t> d_rp_raw;
  vrt::Stage<float> d_rp_depth;
  vrt::Stage<uint32_t> d_rp_out[2];
  vrt::Stage<vrt_pixel_id> d_rp_ids[2];
  int32_t rp_w = 0, rp_h = 0;
  int rp_cur = 0;
  bool rp_valid = false;
  int32_t rp_fetch = VRT_FETCH_NEAREST;  // vrt_set_reprojected_fetch: which filter the loop launches
  float rp_pv[16] = {};
  hipEvent_t ev_rp_beg = nullptr, ev_rp_end = nullptr;
  // vrt_set_reprojected_spatial: the loop's spatial passes (off in a new context), and their staging, allocated
  // with the first frame that runs them: two frames the passes ping-pong through and the filter's tap bytes
  int32_t rp_spatial = VRT_SPATIAL_OFF, rp_sp_passes = 3, rp_sp_guide = VRT_GUIDE_FACE, rp_sp_range = 765;
  vrt::Stage<uint32_t> d_rp_sp[2];
  vrt::Stage<uint8_t> d_rp_taps;
  // first device: staging of the synchronous vrt_spatial_filter: two frames, the IDs and the keep bytes
  vrt::Stage<uint32_t> d_sp_rgba[2];
  vrt::Stage<vrt_pixel_id> d_sp_ids;
  vrt::Stage<uint8_t> d_sp_keep;
  // ABI v12: this process's rank of a one-process-per-GPU job (vrt_comm_join): one RCCL
  // communicator per lane, so that frames in flight on different lane streams gather without
  // ordering each other (a communicator's operations run in issue order)
  std::vector<ncclComm_t> rank_comms;
  int32_t rank_nranks = 0, rank_id = -1;
  std::string err;
};

namespace vrt {

inline int fail(vrt_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

inline int hip_fail(vrt_ctx* c, hipError_t e, const char* what) {
  return fail(c, VRT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

inline int nccl_fail(vrt_ctx* c, ncclResult_t r, const char* what) {
  return fail(c, VRT_ERR_DEVICE, std::string(what) + ": " + ncclGetErrorString(r));
}

#define VRT_HIP(ctx, call)                                   \
  do {                                                       \
    hipError_t e_ = (call);                                  \
    if (e_ != hipSuccess) return hip_fail((ctx), e_, #call); \
  } while (0)

#define VRT_NCCL(ctx, call)                                    \
  do {                                                         \
    ncclResult_t r_ = (call);                                  \
    if (r_ != ncclSuccess) return nccl_fail((ctx), r_, #call); \
  } while (0)

// The caller's current device is restored when an entry point returns (entry points switch
// between the context's devices).
struct DeviceGuard {
  int dev = -1;
  DeviceGuard() { (void)hipGetDevice(&dev); }
  ~DeviceGuard() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
};

// The stream of the shard's one-at-a-time work (volume upload, passes, broadcast): lane 0's first
inline hipStream_t main_stream(const Shard& s) { return s.ls[0][0]; }

// ---- vrt_context.cpp: checks shared by the entry points
int check_render_args(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p);
int check_image(vrt_ctx* ctx, int32_t width, int32_t height);
int check_image(vrt_ctx* ctx, const vrt_camera* cam);
int check_band(vrt_ctx* ctx, int32_t width, int32_t height, int32_t row0, int32_t rows, int64_t pitch,
               bool pitch_first = false);
int check_pixel_list(vrt_ctx* ctx, const vrt_camera* cam, const int32_t* pixels, int32_t count);

// ---- vrt_volume.cpp
int upload_atlas(vrt_ctx* ctx, const uint8_t* rgba, int32_t size);

// ---- vrt_launch.cpp
// How launch() may place a launch's exact pass (launch_state_begin). allow_defer: the launch may defer it
// (frames in flight hide its latency; a frame that runs alone does not). lone: a synchronous whole frame
// that lone_defers: deferred all the same, as one launch with the exact pass's short-band instance.
struct LaunchMode {
  bool allow_defer = true;
  bool lone = false;
};
uint32_t octant_stride(const Shard& s);
KArgs make_args(const vrt_ctx* ctx, const Shard& s, const vrt_camera* cam, const vrt_params* p, int32_t row0,
                int32_t rows, int32_t row_step);
bool lone_defers(const vrt_ctx* ctx, const Shard& s, const KArgs& a);
void launch(const vrt_ctx* ctx, Shard& s, KArgs a, float4* out, vrt_hit* hit, unsigned long long* cnt, hipStream_t st,
            hipEvent_t ev_begin = nullptr, hipEvent_t ev_end = nullptr, LaunchMode mode = LaunchMode());
void launch_timing_events(vrt_ctx* ctx, hipEvent_t& begin, hipEvent_t& end);

// ---- vrt_frames.cpp
int ensure_stage(vrt_ctx* ctx, size_t bytes);

// ---- vrt_queries.cpp: the ID pass, as the filters of vrt_filters.cpp use it
// Arguments shared by vrt_render_ids* and the reprojection (which takes the band's ids and depth), in the pick's
// order. rows / pitch: the band (the synchronous form passes the whole frame's); device: the buffers' alignment is
// checked (the kernels' 8- and 4-byte stores)
int check_ids(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0, int32_t rows, int64_t pitch,
              const void* ids, const void* depth, bool device);
// One ID pass over rows [row0, row0 + rows) (rows >= 1) on `st`: one launch, of the certified ID kernel where
// ids_certified() holds (vrt_set_ids_certified(1) and an octant layout resident), else of the exact ID kernel;
// no allocation, no host synchronisation. d_n_exact (null unless the synchronous vrt_render_ids counts): the
// certified kernel adds its exact-path pixels to that device word; the exact kernel does not touch it
bool ids_certified(const vrt_ctx* ctx);
int enqueue_ids(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* p, int32_t row0, int32_t rows, int32_t pitch,
                vrt_pixel_id* d_ids, float* d_depth, hipStream_t st, uint32_t* d_n_exact = nullptr);

}  // namespace vrt

#pragma GCC visibility pop

#endif  // VRT_CONTEXT_H
