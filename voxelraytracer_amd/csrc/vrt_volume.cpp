// vrt_volume.cpp — the resident volume and atlas of every shard: allocation, upload and broadcast, the
// distance and packing passes, in-place region edits and their plan, device-side scene builds, and the
// packed volume's debug read (vrt_context.h).
#include <cstring>
#include <vector>

#include "vrt_context.h"

namespace vrt {

int upload_atlas(vrt_ctx* ctx, const uint8_t* rgba, int32_t size) {
  if (!rgba || size < 1 || size > 8192 || (size & (size - 1)) != 0)
    return fail(ctx, VRT_ERR_INVALID, "atlas edge must be a power of two in [1, 8192]");
  const size_t bytes = size_t(size) * size * 4;
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    if (s.atlas_size != size) {
      if (s.d_atlas) (void)hipFree(s.d_atlas);
      s.d_atlas = nullptr;
      s.atlas_size = 0;
      if (hipMalloc(&s.d_atlas, bytes) != hipSuccess) return fail(ctx, VRT_ERR_OOM, "hipMalloc atlas");
    }
    VRT_HIP(ctx, hipMemcpy(s.d_atlas, rgba, bytes, hipMemcpyHostToDevice));
    s.atlas_size = size;
  }
  ctx->atlas_host.assign(rgba, rgba + bytes);
  return VRT_OK;
}

static int volume_alloc(vrt_ctx* ctx, Shard& s, int32_t n) {
  if (n < 2 || n > 1024 || (n & (n - 1)) != 0)
    return fail(ctx, VRT_ERR_INVALID, "volume edge must be a power of two in [2, 1024]");
  VRT_HIP(ctx, hipSetDevice(s.device));
  // frames still in flight on the lanes read the resident volume: an upload is not a hot call
  VRT_HIP(ctx, hipDeviceSynchronize());
  // octant layout while 8 padded u16 volumes stay addressable by a 32-bit byte offset
  const bool fits = uint64_t(n + 1) * (n + 1) * (n + 1) * 2 * 8 <= (uint64_t(1) << 32);
  const int32_t octants = fits && ctx->layout_req != 1 ? 8 : 1;
  if (s.d_vox && (s.n != n || s.octants != octants)) {
    (void)hipFree(s.d_vox);
    (void)hipFree(s.d_tmp);
    (void)hipFree(s.d_vox_pad);
    s.d_vox = s.d_tmp = nullptr;
    s.d_vox_pad = nullptr;
  }
  if (!s.d_vox) {
    // (no guard band around the packed volumes: the certified pass's unguarded loads, cert_walk's
    // LEAN forms, only form addresses of cells in [0, N)^3, or texel 0 for a crossing that leaves)
    const size_t bytes = size_t(n) * n * n, pbytes = size_t(n + 1) * (n + 1) * (n + 1) * 2 * size_t(octants);
    if (hipMalloc(&s.d_vox, bytes) != hipSuccess ||
        hipMalloc(&s.d_tmp, (octants == 8 ? 3 : 2) * bytes) != hipSuccess ||
        hipMalloc(&s.d_vox_pad, pbytes) != hipSuccess) {
      if (s.d_vox) (void)hipFree(s.d_vox);
      if (s.d_tmp) (void)hipFree(s.d_tmp);
      if (s.d_vox_pad) (void)hipFree(s.d_vox_pad);
      s.d_vox = s.d_tmp = nullptr;
      s.d_vox_pad = nullptr;
      return fail(ctx, VRT_ERR_OOM, "hipMalloc volume buffers");
    }
  }
  s.n = n;
  s.octants = octants;
  return VRT_OK;
}

static int volume_alloc_all(vrt_ctx* ctx, int32_t n) {
  for (Shard& s : ctx->sh) {
    const int st = volume_alloc(ctx, s, n);
    if (st != VRT_OK) return st;
  }
  return VRT_OK;
}

// certified walks cannot settle glass pixels (their secondary rays start at the exact hit point) and
// a glass pixel pays the certified primary walk before the exact path: the automatic mode turns
// them off when glass makes up more than 1/8 of the non-empty voxels
static void derive_glass_flags(Shard& s) {
  s.cert_auto = s.glass * 8 <= s.non_empty;
  s.has_glass = s.glass > 0;
}

// Distance passes + packing + glass share on every device (canonical bytes already resident on
// each, ordered on part[0]), then wait (upload is not a hot call).
static int volume_finish_all(vrt_ctx* ctx) {
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    const uint64_t vol = uint64_t(s.n) * s.n * s.n;
    // the whole volume as one edit box: every texel of the packed volume(s) is rebuilt
    const int32_t origin[3] = {0, 0, 0}, extent[3] = {s.n, s.n, s.n};
    vrt::launch_volume_edit_passes(s.d_vox, s.d_tmp, s.d_vox_pad, uint32_t(s.n), s.octants, origin, extent, true,
                                   main_stream(s));
    if (!s.d_vstats) VRT_HIP(ctx, hipMalloc(&s.d_vstats, kVstatWords * sizeof(unsigned long long)));
    VRT_HIP(ctx, hipMemsetAsync(s.d_vstats, 0, 2 * sizeof(unsigned long long), main_stream(s)));
    vrt::launch_glass_share(s.d_vox, vol, s.d_vstats, main_stream(s));
    VRT_HIP(ctx, hipGetLastError());
  }
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    unsigned long long vs[2] = {0, 0};
    VRT_HIP(ctx, hipMemcpyAsync(vs, s.d_vstats, sizeof(vs), hipMemcpyDeviceToHost, main_stream(s)));
    VRT_HIP(ctx, hipStreamSynchronize(main_stream(s)));
    s.glass = vs[0];
    s.non_empty = vs[1];
    derive_glass_flags(s);
  }
  ctx->err.clear();
  return VRT_OK;
}

// vrt_update_volume_region / _device: the box from the host (`host`) or from the first device
// (`dev`, ordered on cs) to every device, which writes it into its canonical replica and rebuilds
// the packed texels of the edit plan (launch_volume_edit_passes).
static int update_region_all(vrt_ctx* ctx, const int32_t origin[3], const int32_t extent[3], const uint8_t* host,
                      const uint8_t* dev, hipStream_t cs) {
  Shard& root = ctx->sh[0];
  if (!root.d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  if (!origin || !extent || (!host && !dev)) return fail(ctx, VRT_ERR_INVALID, "null origin, extent or voxels");
  for (int a = 0; a < 3; ++a) {
    if (extent[a] <= 0) return fail(ctx, VRT_ERR_INVALID, "edit extent must be positive");
    if (origin[a] < 0 || origin[a] >= root.n || extent[a] > root.n - origin[a])
      return fail(ctx, VRT_ERR_INVALID, "edit box is not inside the volume");
  }
  const size_t bytes = size_t(extent[0]) * size_t(extent[1]) * size_t(extent[2]);
  DeviceGuard guard;
  // frames still in flight on the lanes read the packed volume (the upload's rule)
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    VRT_HIP(ctx, hipDeviceSynchronize());
  }
  if (dev) {
    VRT_HIP(ctx, hipSetDevice(root.device));
    VRT_HIP(ctx, hipEventRecord(root.ev_gs, cs));
  }
  // the box is staged at the head of d_tmp (bytes <= N^3), which the passes only write after the
  // box write has read it
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    if (dev) {
      VRT_HIP(ctx, hipStreamWaitEvent(main_stream(s), root.ev_gs, 0));
      VRT_HIP(ctx, hipMemcpyPeerAsync(s.d_tmp, s.device, dev, root.device, bytes, main_stream(s)));
    } else {
      VRT_HIP(ctx, hipMemcpyAsync(s.d_tmp, host, bytes, hipMemcpyHostToDevice, main_stream(s)));
    }
    VRT_HIP(ctx, hipMemsetAsync(s.d_vstats, 0, kVstatWords * sizeof(unsigned long long), main_stream(s)));
    vrt::launch_edit_apply(s.d_tmp, s.d_vox, uint32_t(s.n), origin, extent, s.d_vstats, main_stream(s));
    VRT_HIP(ctx, hipGetLastError());
  }
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    unsigned long long c[5] = {0, 0, 0, 0, 0};
    VRT_HIP(ctx, hipMemcpyAsync(c, s.d_vstats, sizeof(c), hipMemcpyDeviceToHost, main_stream(s)));
    VRT_HIP(ctx, hipStreamSynchronize(main_stream(s)));
    s.glass = s.glass - c[0] + c[2];
    s.non_empty = s.non_empty - c[1] + c[3];
    derive_glass_flags(s);
    // no cell became empty or occupied: every skip distance stands, only voxel bytes change
    vrt::launch_volume_edit_passes(s.d_vox, s.d_tmp, s.d_vox_pad, uint32_t(s.n), s.octants, origin, extent,
                                   c[4] != 0, main_stream(s));
    VRT_HIP(ctx, hipGetLastError());
  }
  for (Shard& s : ctx->sh) {
    VRT_HIP(ctx, hipSetDevice(s.device));
    VRT_HIP(ctx, hipStreamSynchronize(main_stream(s)));
  }
  ctx->err.clear();
  return VRT_OK;
}

// The first device's canonical volume (resident, ordered on its part[0]) to every other device:
// ncclBroadcast over xGMI, or device-to-device copies when a device repeats.
static int broadcast_volume(vrt_ctx* ctx) {
  const size_t k = ctx->sh.size();
  if (k == 1 && !ctx->coll1) return VRT_OK;
  Shard& root = ctx->sh[0];
  const size_t bytes = size_t(root.n) * root.n * root.n;
  if (ctx->distinct) {
    VRT_NCCL(ctx, ncclGroupStart());
    for (size_t j = 0; j < k; ++j) {
      Shard& s = ctx->sh[j];
      (void)hipSetDevice(s.device);
      const ncclResult_t r = ncclBroadcast(root.d_vox, s.d_vox, bytes, ncclUint8, 0, ctx->comms[j], main_stream(s));
      if (r != ncclSuccess) {
        (void)ncclGroupEnd();
        return nccl_fail(ctx, r, "ncclBroadcast(volume)");
      }
    }
    VRT_NCCL(ctx, ncclGroupEnd());
    return VRT_OK;
  }
  VRT_HIP(ctx, hipSetDevice(root.device));
  VRT_HIP(ctx, hipEventRecord(root.ev_gs, main_stream(root)));
  for (size_t j = 1; j < k; ++j) {
    Shard& s = ctx->sh[j];
    VRT_HIP(ctx, hipSetDevice(s.device));
    VRT_HIP(ctx, hipStreamWaitEvent(main_stream(s), root.ev_gs, 0));
    VRT_HIP(ctx, hipMemcpyPeerAsync(s.d_vox, s.device, root.d_vox, root.device, bytes, main_stream(s)));
  }
  return VRT_OK;
}

}  // namespace vrt

using namespace vrt;

extern "C" {

int vrt_upload_volume(vrt_ctx* ctx, const vrt_volume* vol) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!vol || !vol->voxels) return fail(ctx, VRT_ERR_INVALID, "null volume");
  DeviceGuard guard;
  int st = volume_alloc_all(ctx, vol->n);
  if (st != VRT_OK) return st;
  Shard& root = ctx->sh[0];
  const size_t bytes = size_t(vol->n) * vol->n * vol->n;
  VRT_HIP(ctx, hipSetDevice(root.device));
  VRT_HIP(ctx, hipMemcpyAsync(root.d_vox, vol->voxels, bytes, hipMemcpyHostToDevice, main_stream(root)));
  if ((st = broadcast_volume(ctx)) != VRT_OK) return st;
  return volume_finish_all(ctx);
}

int vrt_upload_volume_device(vrt_ctx* ctx, const uint8_t* d_voxels, int32_t n, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!d_voxels) return fail(ctx, VRT_ERR_INVALID, "null volume");
  DeviceGuard guard;
  int st = volume_alloc_all(ctx, n);
  if (st != VRT_OK) return st;
  Shard& root = ctx->sh[0];
  const size_t bytes = size_t(n) * n * n;
  VRT_HIP(ctx, hipSetDevice(root.device));
  // ordered after the caller's work on hip_stream (which produced d_voxels)
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  VRT_HIP(ctx, hipMemcpyAsync(root.d_vox, d_voxels, bytes, hipMemcpyDeviceToDevice, s));
  VRT_HIP(ctx, hipEventRecord(root.ev_gs, s));
  VRT_HIP(ctx, hipStreamWaitEvent(main_stream(root), root.ev_gs, 0));
  if ((st = broadcast_volume(ctx)) != VRT_OK) return st;
  return volume_finish_all(ctx);
}

int vrt_update_volume_region(vrt_ctx* ctx, const int32_t origin[3], const int32_t extent[3], const uint8_t* voxels) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!voxels) return fail(ctx, VRT_ERR_INVALID, "null voxels");
  return update_region_all(ctx, origin, extent, voxels, nullptr, nullptr);
}

int vrt_update_volume_region_device(vrt_ctx* ctx, const int32_t origin[3], const int32_t extent[3],
                                    const uint8_t* d_voxels, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (!d_voxels) return fail(ctx, VRT_ERR_INVALID, "null voxels");
  return update_region_all(ctx, origin, extent, nullptr, d_voxels, static_cast<hipStream_t>(hip_stream));
}

int vrt_volume_edit_plan(int32_t n, int32_t octants, const int32_t origin[3], const int32_t extent[3], int32_t* out) {
  if (!origin || !extent || !out || (octants != 8 && octants != 1) || n < 2 || n > 1024 || (n & (n - 1)) != 0)
    return VRT_ERR_INVALID;
  for (int a = 0; a < 3; ++a)
    if (extent[a] <= 0 || origin[a] < 0 || origin[a] >= n || extent[a] > n - origin[a]) return VRT_ERR_INVALID;
  return vrt::volume_edit_plan(n, octants, origin, extent, out);
}

int vrt_build_scene_device(vrt_ctx* ctx, int32_t scene, int32_t n, uint32_t seed, void* hip_stream) {
  if (!ctx) return VRT_ERR_INVALID;
  if (scene != VRT_SCENE_TERRAIN && scene != VRT_SCENE_GLASS_CUBE && scene != VRT_SCENE_REFRACTION)
    return fail(ctx, VRT_ERR_INVALID, "unknown scene");
  if (n < 8) return fail(ctx, VRT_ERR_INVALID, "scene edge must be >= 8");
  DeviceGuard guard;
  const int st = volume_alloc_all(ctx, n);
  if (st != VRT_OK) return st;
  std::vector<float> noise;
  if (scene == VRT_SCENE_TERRAIN) {  // the heightfield (n*n floats) is built on the host
    noise.resize(size_t(n) * n);
    if (vrt_terrain_noise(n, seed, noise.data()) != VRT_OK) return fail(ctx, VRT_ERR_INVALID, "noise");
  }
  hipStream_t cs = static_cast<hipStream_t>(hip_stream);
  for (Shard& s : ctx->sh) {  // every device builds its own replica: no transfer
    VRT_HIP(ctx, hipSetDevice(s.device));
    const float* d_noise = nullptr;
    if (!noise.empty()) {
      // d_tmp (>= 2 N^3 bytes >= 4 N^2) is free until the distance passes
      VRT_HIP(ctx, hipMemcpyAsync(s.d_tmp, noise.data(), noise.size() * sizeof(float),
                                  hipMemcpyHostToDevice, main_stream(s)));
      d_noise = reinterpret_cast<const float*>(s.d_tmp);
    }
    if (&s == &ctx->sh[0] && cs) {  // ordered after the caller's prior work on its stream
      VRT_HIP(ctx, hipEventRecord(s.ev_gs, cs));
      VRT_HIP(ctx, hipStreamWaitEvent(main_stream(s), s.ev_gs, 0));
    }
    vrt::launch_build_scene(s.d_vox, scene, uint32_t(n), d_noise, main_stream(s));
    VRT_HIP(ctx, hipGetLastError());
  }
  return volume_finish_all(ctx);
}

const uint8_t* vrt_volume_device_ptr(const vrt_ctx* ctx) { return ctx ? ctx->sh[0].d_vox : nullptr; }

int vrt_debug_packed_volume(vrt_ctx* ctx, uint16_t* out, uint64_t count) {
  if (!ctx) return VRT_ERR_INVALID;
  Shard& s = ctx->sh[0];
  if (!s.d_vox_pad) return fail(ctx, VRT_ERR_NO_VOLUME, "no volume uploaded");
  const uint64_t p = uint64_t(s.n) + 1, total = p * p * p * uint64_t(s.octants);
  if (!out || count < total) return fail(ctx, VRT_ERR_INVALID, "output smaller than octants x (N+1)^3");
  DeviceGuard guard;
  VRT_HIP(ctx, hipSetDevice(s.device));
  VRT_HIP(ctx, hipMemcpy(out, s.d_vox_pad, total * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return VRT_OK;
}

int vrt_upload_atlas(vrt_ctx* ctx, const uint8_t* rgba, int32_t atlas_size) {
  if (!ctx) return VRT_ERR_INVALID;
  DeviceGuard guard;
  const int st = upload_atlas(ctx, rgba, atlas_size);
  if (st == VRT_OK) ctx->err.clear();
  return st;
}

}  // extern "C"
