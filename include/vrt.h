/*
 * vrt.h — C-ABI drop-in boundary of the MI355X-native voxel ray tracer.
 *
 * Replaces the reference's GL boundary for the per-pixel ray-trace pass:
 *   - 3D-texture upload      src/main.cpp:315-319  (glTexImage3D GL_RED/UNSIGNED_BYTE, NEAREST)
 *   - uniforms + quad draw    src/main.cpp:325-361  (u_PVInvMatrix, u_Size, u_SunDir, u_Time, noises)
 *   - RGB colour FBO          src/FrameBuffer.cpp:5-19
 * and executes the program in res/shaders/voxel.glsl (fragment :1-452, vertex :454-475)
 * as a hand-written gfx950 HIP kernel.
 *
 * Conventions
 *   - Plain C types only; no exceptions cross the ABI; every entry point returns a vrt_status
 *     (0 = ok, <0 = error) and sets a per-context message readable with vrt_last_error().
 *   - Not thread-safe per context: one context per host thread (as the GL context was).
 *   - Volumes are N^3 bytes, x fastest: idx = x + y*N + z*N*N   (main.cpp:227).
 *   - Images are W*H RGBA float, row 0 = bottom row (GL window convention).
 *   - A context spans one or more GPUs (vrt_create's device mask). Whole-frame entry points
 *     (vrt_render, vrt_render_frame, vrt_render_frame_device) split the frame over k > 1 devices
 *     into block-cyclic bands of 16 adjacent rows (ABI v12; device j renders row blocks j, j+k,
 *     ..., one launch per band; vrt_frame_row_block), rendered on context-owned streams: frame f
 *     on lane f % 4. On one device a frame that runs alone (synchronous calls) or reads its
 *     history is two interleaved row parts on two streams (a synchronous colour-only certified
 *     frame of a glass-heavy volume or of >= 8 rounds of resident waves: one deferred launch, see
 *     vrt_set_exact_pass); a device-output frame at u_Alpha = 1
 *     is one launch, and up to four frames are in flight (ABI v9). The *_async band entry points
 *     run on the context's first (root) device, as do the ray queries (vrt_cast_rays*,
 *     vrt_pick_pixels: which voxel a ray meets), the shaded ray queries (vrt_trace_rays*,
 *     vrt_trace_pixels: which colour a ray sees), the ID and depth pass (vrt_render_ids*: which
 *     voxel and face every pixel shows, and how far away), the reprojected temporal filter
 *     (vrt_reproject_temporal_async, vrt_render_frame_reprojected: a history that follows the camera)
 *     and the ID-guided spatial filter (vrt_spatial_filter*: an estimate for a pixel without history).
 */
#ifndef VRT_H
#define VRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VRT_ABI_VERSION 15

typedef struct vrt_ctx vrt_ctx;

typedef enum {
  VRT_OK = 0,
  VRT_ERR_INVALID = -1,      /* bad argument (null pointer, size, unsupported N) */
  VRT_ERR_DEVICE = -2,       /* HIP runtime error (message has the hipError string) */
  VRT_ERR_NO_VOLUME = -3,    /* vrt_render before vrt_upload_volume */
  VRT_ERR_OOM = -4,          /* device allocation failed */
  VRT_ERR_UNSUPPORTED = -5   /* parameter combination not built (see vrt_last_error) */
} vrt_status;

/* Camera: u_PVInvMatrix (voxel.glsl:464, set at main.cpp:333) plus the FBO size. */
typedef struct {
  float inv_pv[16];   /* column-major, GL convention: m[col*4 + row] */
  int32_t width;
  int32_t height;
} vrt_camera;

/* Volume: the bytes main.cpp:218-288 builds and :318 uploads. */
typedef struct {
  const uint8_t* voxels; /* host pointer, N^3 bytes, x fastest */
  int32_t n;             /* u_Size (voxel.glsl:18) */
} vrt_volume;

/* Per-frame parameters: the remaining uniforms (main.cpp:335-348) and compile-time switches. */
typedef struct {
  float sun_dir[3];           /* u_SunDir (main.cpp:346-348); the shader re-normalises it */
  float time;                 /* u_Time, the frame counter as float (main.cpp:343-345) */
  float ray_noise;            /* u_RayNoise        [0, 0.05] */
  float reflection_noise;     /* u_ReflectionNoise [0, 0.05] */
  float refraction_noise;     /* u_RefractionNoise [0, 0.01] */
  float max_ray_length;       /* u_MaxRayLength, default 100 (voxel.glsl:17) */
  int32_t max_reflections;    /* MAX_REFLECTIONS   (voxel.glsl:4), 0..8 */
  int32_t max_transparencies; /* MAX_TRANSPARENCIES (voxel.glsl:5), 0..8 */
  int32_t color_only;         /* _COLOR_ONLY (voxel.glsl:6): 1 colour-only, 0 textured */
  int32_t reserved0;
  const uint8_t* atlas_rgba;  /* textured mode: u_TextureUnit atlas (see vrt_upload_atlas) */
  int32_t atlas_size;         /* u_AtlasSize */
  int32_t atlas_texture_size; /* u_AtlasTextureSize */
} vrt_params;

/* Per-pixel record of the PRIMARY ray (the first stack pop, voxel.glsl:430-437). Parity key:
 * bit-exact between the HIP kernel and the CPU oracle. */
typedef struct {
  int32_t voxel_index;  /* linear index of the hit voxel (the texel GetVoxel read), -1 = no hit */
  float ray_length;     /* RayIntersection.rayLength of the primary hit (0 if none) */
  uint32_t steps;       /* DDA + shadow-DDA iterations spent on the whole pixel */
  uint32_t flags;       /* VRT_HIT_FLAG_* */
} vrt_hit;

#define VRT_HIT_FLAG_TIE3 1u        /* a y+z (or x+y+z) zero-t tie read intersectionAxis[3] (clamped to 2) */
#define VRT_HIT_FLAG_STEP_CAP 2u    /* a march hit VRT_MAX_STEPS (the GLSL would spin) */
#define VRT_HIT_FLAG_STACK_FULL 4u  /* a push was dropped (cannot happen for stack = R+T+1) */

#define VRT_MAX_STEPS 4096          /* per RayMarch / RayMarchShadow call */

/* Counter slots (uint64 each) accumulated by a render. Algorithmic bytes of a frame:
 *   DDA_STEPS + SHADOW_STEPS + 2*REFRACTION_PROBES + 16*PIXELS */
enum {
  VRT_CNT_PIXELS = 0,
  VRT_CNT_PRIMARY_RAYS,
  VRT_CNT_SECONDARY_RAYS,     /* stack pops after the primary */
  VRT_CNT_SHADOW_RAYS,        /* RayMarchShadow calls */
  VRT_CNT_DDA_STEPS,          /* RayMarch iterations that called GetVoxel */
  VRT_CNT_SHADOW_STEPS,       /* RayMarchShadow iterations that called GetVoxel */
  VRT_CNT_REFRACTION_PROBES,  /* GetRefractionRay calls (2 voxel reads each) */
  VRT_CNT_TIE3,               /* index==3 tie events */
  VRT_CNT_STEP_CAP,           /* marches cut by VRT_MAX_STEPS */
  VRT_CNT_COUNT
};

/* Statistics of a synchronous render. kernel_ms is always filled: the GPU time of the frame's
 * launches (hipEvents, the max over the context's devices), like the reference's GL_TIME_ELAPSED
 * query (main.cpp:350-360). Counters are filled only when requested (request |=
 * VRT_STATS_COUNTERS): counting runs the exact-walk instance, ~3x slower than the uncounted
 * frame, so timing alone never asks for it. */
#define VRT_STATS_COUNTERS 1u
typedef struct {
  uint64_t counters[VRT_CNT_COUNT];  /* out (when requested) */
  float kernel_ms;                   /* out */
  uint32_t request;                  /* in: VRT_STATS_* bits */
  float reserved[2];
} vrt_stats;

/* ---- context / device ---------------------------------------------------------------------- */

/* Create a context on the HIP devices of `device_mask` (bit i = device ordinal i):
 * one device renders whole frames; k devices split every whole frame into k block-cyclic bands
 * (ABI v12: device j of the mask renders the 16-row blocks j, j+k, ...; until v11 cyclic rows j,
 * j+k, ...; the volume is replicated on every device: RCCL broadcast from the first device, RCCL
 * communicators over the mask's devices). */
int vrt_create(uint32_t device_mask, vrt_ctx** out);
/* Same over an explicit device list; a device may repeat (rehearses a k-device split on fewer
 * GPUs: the bands and the gather then use device-to-device copies instead of RCCL). */
int vrt_create_devices(const int32_t* devices, int32_t count, vrt_ctx** out);
/* Devices of the context (k), and the ordinal of its i-th device (-1 if out of range). */
int vrt_device_count(const vrt_ctx* ctx);
int vrt_device_ordinal(const vrt_ctx* ctx, int32_t i);
void vrt_destroy(vrt_ctx* ctx);
const char* vrt_last_error(const vrt_ctx* ctx);  /* never NULL; "" when no error */
int vrt_abi_version(void);

/* Copy the volume to device memory (replaces glTexImage3D, main.cpp:315-318): host -> the first
 * device, then a broadcast to the others. The caller keeps ownership of `vol->voxels`. N must be
 * a power of two in [2, 1024]. */
int vrt_upload_volume(vrt_ctx* ctx, const vrt_volume* vol);

/* Same from a DEVICE buffer of N^3 bytes on the context's first GPU (e.g. after an RCCL broadcast
 * of the volume to every GPU of the node by the caller), ordered on `hip_stream`; the context's
 * other devices receive it by broadcast; returns after the copy. */
int vrt_upload_volume_device(vrt_ctx* ctx, const uint8_t* d_voxels, int32_t n, void* hip_stream);

/* Build the _TERRAIN / _GLASS_CUBE / _REFRACTION volume of main.cpp:218-288 directly on the device
 * (bytes identical to vrt_build_scene; only the n*n terrain heightfield is computed on the host)
 * and make it the context's volume, ordered on `hip_stream`; returns after the build. N must be
 * a power of two in [8, 1024]. Replaces the host build + glTexImage3D upload (main.cpp:315-318).
 * Every device of the context builds its own replica (no transfer). */
int vrt_build_scene_device(vrt_ctx* ctx, int32_t scene, int32_t n, uint32_t seed, void* hip_stream);

/* Added within v15 (detect by symbol lookup): in-place voxel edits, the glTexSubImage3D of this
 * boundary. Replace the voxels of the box [origin, origin+extent) of the resident volume with
 * `voxels` (host, extent[0]*extent[1]*extent[2] bytes, x fastest inside the box) and bring every
 * packed skip-distance volume, on every device of the context, to exactly the bytes a full
 * vrt_upload_volume of the edited volume would produce. Skip distances have bounded support (the
 * forward distance is capped at 128, the centred one at 64), so only the packed texels of
 * vrt_volume_edit_plan's boxes are rebuilt, by region passes in the resident scratch: the call
 * allocates nothing, and the layout, N and the octant count stay. An edit that changes no cell's
 * emptiness (materials only) rewrites the box's voxel bytes alone. The glass share behind
 * vrt_set_certified's automatic mode moves by the box's counts, so vrt_certified() equals that of a
 * fresh upload. Ordering is the upload's: the call waits for the frames in flight on the context's
 * lanes (they read the packed volume) and returns when the edit is complete on every device.
 * VRT_ERR_NO_VOLUME without a resident volume; VRT_ERR_INVALID for null pointers, an extent <= 0
 * or a box not inside [0, N)^3; a failed call leaves the volume as it was. */
int vrt_update_volume_region(vrt_ctx* ctx, const int32_t origin[3], const int32_t extent[3],
                             const uint8_t* voxels);
/* Same from a DEVICE buffer on the context's first device, ordered on `hip_stream`; the other
 * devices receive the box by peer copies. */
int vrt_update_volume_region_device(vrt_ctx* ctx, const int32_t origin[3], const int32_t extent[3],
                                    const uint8_t* d_voxels, void* hip_stream);
/* Added within v15. Host arithmetic, no GPU (like vrt_block_band_plan): per packed volume
 * o < octants (8 or 1; bit a of o: the octant's step on axis a is -1), out[o*6+0..5] =
 * {x0,y0,z0,x1,y1,z1}, the half-open box of packed texels in [0, N)^3 that an edit of the box
 * [origin, origin+extent) = [lo, hi) may change. Octants, per axis with step s: the anchors whose
 * forward distance F can change are [lo-127, hi-1] (s = +1) or [lo, hi-1+127] (s = -1), the texel
 * G(w) = F(w - s) - 1 shifts them by s, the edit's own cells join for the voxel bytes, and the
 * result is clipped to [0, N). Single layout: [lo-63, hi-1+63] per axis, clipped. (Texels at
 * coordinate N, which repeat voxel 0, are rewritten besides when the box holds coordinate 0.)
 * Returns octants, or VRT_ERR_INVALID (null pointers, octants not 8 or 1, N not a power of two in
 * [2, 1024], a box not inside the volume). */
int vrt_volume_edit_plan(int32_t n, int32_t octants, const int32_t origin[3], const int32_t extent[3],
                         int32_t* out);

/* Device pointer of the resident volume (N^3 bytes, canonical layout), e.g. for a broadcast.
 * NULL if none. An edit (vrt_update_volume_region) updates it in place. */
const uint8_t* vrt_volume_device_ptr(const vrt_ctx* ctx);

/* Diagnostic: copy the kernel's device volume to `out` (count >= octants x (N+1)^3, see
 * vrt_volume_octants): per octant o (bit 0: dir.x < 0, bit 1: dir.y < 0, bit 2: dir.z < 0), a padded
 * (N+1)^3 u16 volume = voxel | G << 8 (x fastest; plane N repeats plane 0 with G = 0). Octant
 * layout (N <= 512): G(v) = F(v - s) - 1, F(u) = edge of the largest empty in-volume cube anchored
 * at u extending along s = the octant's step (capped at 64). Single layout (N = 1024): G = the
 * Chebyshev distance to the nearest non-empty voxel or the volume outside, capped at 64.
 * Synchronous. */
int vrt_debug_packed_volume(vrt_ctx* ctx, uint16_t* out, uint64_t count);

/* ABI v5: number of packed volumes of the resident volume (8 octant volumes, or 1 for N = 1024;
 * 0 when none is uploaded). */
int vrt_volume_octants(const vrt_ctx* ctx);

/* ABI v5: skip-distance layout of the NEXT volume upload: 0 = automatic (8 octant volumes for
 * N <= 512, else 1), 1 = one volume with the centred Chebyshev distance (the N = 1024 layout, at
 * any N: tests and A/B timing), 8 = octant volumes where they fit. Images are identical. */
int vrt_set_skip_layout(vrt_ctx* ctx, int32_t octants);

/* ABI v6: certified walks for stats-free colour-only frames (DESIGN.md §6 "Certified walks"): a
 * pixel whose primary outcome and shadow bit provably equal the exact walks' is shaded from a
 * few empty-space jumps; every other pixel (glass hits, near-edge crossings) takes the exact walk,
 * whose shadow rays and air-medium secondary rays are again certified walks when they can be.
 * mode 1 = always, -1 = never (exact walks only), 0 = automatic (default): with the octant layout,
 * certified pixels unless glass makes up more than 1/8 of the resident volume's non-empty voxels
 * (glass pixels pay the certified primary walk before the exact path), certified exact-path rays
 * always. Frames with hit records or counters and textured frames always take the exact walks.
 * Images are identical in every mode. */
int vrt_set_certified(vrt_ctx* ctx, int32_t mode);

/* ABI v6: 1 when the next stats-free colour-only frame tries certified walks for whole pixels,
 * else 0. */
int vrt_certified(const vrt_ctx* ctx);

/* ABI v8 (r02): device timestamps of the async band launches (vrt_render_rows*_async,
 * vrt_render_temporal_rows*_async on the first device) and of the ray-query launches (vrt_cast_rays*,
 * vrt_pick_pixels, vrt_trace_rays*, vrt_trace_pixels, vrt_render_ids*, vrt_reproject_temporal_async,
 * vrt_reproject_temporal_fetch_async: one launch per call):
 * vrt_set_launch_timing(ctx, n) creates
 * timing events for the next n launches (0: off; it synchronises the first device when replacing
 * earlier events), each launch then records its kernel's start and end on the device
 * (hipExtLaunchKernelGGL); vrt_launch_timing waits for the recorded launches, returns the sum of
 * their kernel durations and their count, and frees the events for the next n launches. This is
 * the per-kernel duration a profiler reports, measured in the caller's own timed region. */
int vrt_set_launch_timing(vrt_ctx* ctx, int32_t launches);
int vrt_launch_timing(vrt_ctx* ctx, double* total_ms, uint64_t* launches);

/* ABI v7: heavy-first tile order for stats-free colour-only launches with certified pixels
 * (vrt_certified() == 1) of volumes with glass (DESIGN.md §6 "Tile order"): on = 1 (default),
 * off = 0. ABI v14: 1 is automatic, launches of at least one dispatch round of resident waves
 * (CUs x 4 x 7: 7168 waves, e.g. 1920 x 240 pixels, on MI355X; smaller launches have every tile
 * resident at once, so the order would only cost its bookkeeping), 2 = every launch. Each launch records which of its 16x8 tiles had a pixel on the exact path (glass
 * bounce stacks, near-edge walks; until ABI v8 only bounce stacks); the next launch of the same
 * band (width, rows, row0, row_step) on the same stream dispatches those tiles first, each on the
 * same XCD as before, the last to finish first, so the frame's longest waves start first.
 * Launches on a stream that is being captured into a graph use dispatch order. Every tile is
 * rendered exactly once in any case: images are identical with and without it.
 * ABI v8: the state is a pool allocated by vrt_create (ABI v9: 16 slots of 5 x 65536 words + a
 * header; since v14 5 x 131072 words: launches up to 131072 tiles, i.e. 4096 x 4096 pixels; larger
 * launches use dispatch order), a
 * slot per (band, stream), zeroed on the launch stream when it is (re)assigned. Reassigning the
 * least recently used slot (more than 16 band/stream pairs in use) synchronises the device once
 * (ABI v9: the old stream is never touched; its owner may have destroyed it). */
int vrt_set_tile_order(vrt_ctx* ctx, int32_t on);

/* ABI v9: deferred exact pass for stats-free launches with certified pixels (vrt_certified() == 1):
 * on = 1 (default, automatic) or 2 (always, whatever the band size: tests and A/B timing): the
 * certified pass renders the pixels its certified walks settle and appends the others (glass hits,
 * near-edge walks, textured hits near a texel edge) to a list, in 8 segments by column block of the
 * band (ABI v13; spatially coherent batches); a second kernel on the same stream renders them with
 * the exact path: a wave's own >= 32 pixels as one chunk, the rest 32 to a wave (16 in short bands).
 * It pays when other work overlaps the exact pass and the launch is large: the async band entry
 * points and the device-output frames (frames in flight) use it for bands of at least two rounds of
 * resident waves (CUs x 4 x 7 x 2 waves: 14336, e.g. 1920 x 960 pixels, on MI355X); smaller bands
 * and the synchronous whole-frame calls (vrt_render, vrt_render_frame) keep the in-lane path, except
 * a synchronous colour-only frame (u_Alpha = 1 for vrt_render_frame) of a glass-heavy volume or of
 * >= 8 rounds of resident waves, which is one deferred launch with the exact pass's short-band
 * instance (its in-lane alternative waits on the glass trees, or the long certified pass carries
 * the exact pass's tail; C1 0.330 -> 0.25 ms, C4 0.247 -> 0.21). off =
 * 0: the exact path runs in the pixel's own lane, with the heavy-first tile order
 * (vrt_set_tile_order). Launches over 131072 tiles, and launches on a stream being captured into a
 * graph, use the in-lane path. Images are identical either way. */
int vrt_set_exact_pass(vrt_ctx* ctx, int32_t on);

/* ABI v15: certified bounce trees for stats-free colour-only frames with certified pixels
 * (DESIGN.md §6 "Certified bounce trees"): 1 = automatic (default), 2 = always, 0 = off. A pixel
 * whose primary ray hits glass has its whole bounce tree (voxel.glsl:425-452) walked by certified
 * walks from the certified hits' uncertain origins, the colour folded in the reference's order;
 * any ray whose walk, start or direction could differ from the exact path's sends the pixel to the
 * exact path (deferred or in lane, as above). The certified pass that runs the trees is its own
 * kernel instance (more registers per lane); automatic mode uses it for the volumes whose glass is
 * more than 1/8 of the non-empty voxels, where the automatic certified mode (vrt_set_certified 0)
 * would otherwise render every pixel exactly, so the certified mode is then on for them too; in
 * glass-light volumes the few glass pixels keep the deferred exact path. Images are identical in
 * every mode. */
int vrt_set_cert_trees(vrt_ctx* ctx, int32_t on);

/* Diagnostic: the kernel's RandomizeDirection (voxel.glsl:132-140) for n (dir, pos) float3
 * pairs, out = n float3. Synchronous. */
int vrt_debug_randomize(vrt_ctx* ctx, const float* dir, const float* pos, int32_t n,
                        float randomness, float seed, float* out);

/* Added within v15 (detect by symbol lookup). Diagnostic: one certified walk per listed ray
 * on the resident volume, which must have the eight-octant skip layout (vrt_volume_octants() == 8).
 * rays: `count` (<= 2^24) records of 32 bytes, vrt_ray's layout with the reserved word read as float len0,
 * the ray's length so far (0 <= len0 <= 1e4, |max_length| <= 1e4), origins in volume coordinates.
 * kind: 0 the walk of a ray in air from an exact origin, 1 the shadow walk along the ray's own direction,
 * 2 and 3 the same two walks in the certified pass's form (its unguarded loads). out: `count` records of
 * 32 bytes: int32 res (0 a certified miss, 1 a certified hit, 2 unsure, 3 not started: the ray's
 * direction, start cell or start layers do not allow a certified walk), uint32 byte, int32 axis, int32 cell
 * x, y, z of the hit, float u, the hit's parameter along the ray, and float eu, the bound of the exact
 * walk's parameter error there (byte to eu mean something for res 1). Host pointers. Synchronous. */
int vrt_debug_cert_walks(vrt_ctx* ctx, const void* rays, int64_t count, int32_t kind, void* out);

/* Diagnostic: the kernels' fast correctly rounded reciprocal (the hardware reciprocal plus one
 * Newton step) and square root (the hardware square root plus its residual fix) checked against
 * the IEEE division and square root over all 2^32 float bit patterns on the context's first
 * device. out[7]: patterns the kernels take the reciprocal for, mismatches among them (must be 0),
 * mismatches of normal-range patterns with an all-ones significand and of the remaining non-NaN
 * patterns (both take the division), the first mismatching pattern of the first kind (~0 if none),
 * positive patterns the kernels take the square root for, mismatches among them (must be 0).
 * Synchronous. */
int vrt_debug_fast_math(vrt_ctx* ctx, uint64_t* out);

/* Added within v15 (detect by symbol lookup). Diagnostic: the two power forms the certified pass relies
 * on, over all 2^32 float bit patterns x on the context's first device. out[6]:
 * (a) the skybox's sun disc 10 * pow(x, 400) by the library's log2 and exp2: out[0] = patterns x in
 *     [-0, 0.75] (the sign bit alone, or 0 <= x <= 0.75), out[1] = those among them whose result is not +0,
 *     out[2] = patterns with x < 0 or NaN, out[3] = those among them whose result is no NaN;
 * (b) the specular power pow(max(x, 0), 10) by the library's forms and by the bare hardware log and exp:
 *     out[4] = patterns whose two results differ in their bits while either is at least 2^-100 in magnitude
 *     (or a NaN), out[5] = the first such pattern (~0 if none).
 * out[1], out[3] and out[4] must be 0. Synchronous. */
int vrt_debug_pow_forms(vrt_ctx* ctx, uint64_t* out);

/* Diagnostic (test rehearsal of the multi-GPU path on a one-GPU box): a one-device context takes
 * the k-device path through RCCL with a one-rank communicator (ncclCommInitAll over its device):
 * the volume upload goes through ncclBroadcast (in place) and vrt_render_frame_device through
 * ncclGather of the band into the gather buffer and the strided assembly copy, as with k distinct
 * GPUs. Call once, right after vrt_create with one device; frames are identical either way. */
int vrt_debug_collectives(vrt_ctx* ctx);

/* Synchronous whole-frame render (replaces main.cpp:325-361): writes W*H RGBA floats
 * (alpha = 1, voxel.glsl:451) to the HOST buffer out_rgba. out_hit (W*H records) and stats may
 * be NULL. Hit records or counters run the exact-walk instance; otherwise the fast instance on
 * the context's streams. Each device copies its band straight into the host rows. */
int vrt_render(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
               float* out_rgba, vrt_hit* out_hit, vrt_stats* stats);

/* Asynchronous band render into DEVICE buffers on `hip_stream` (hipStream_t, NULL = default).
 * Renders frame rows row0 + i*row_step for i in [0, rows) at full width; output row i of
 * d_out_rgba / d_out_hit holds frame row row0 + i*row_step. d_out_hit and d_counters
 * (VRT_CNT_COUNT uint64, ACCUMULATED into; the caller zeroes them) may be NULL. Counting uses a
 * per-context replica buffer: at most one counted render per context in flight at a time.
 * No host sync, no allocation: capturable in a hipGraph (the tile order is skipped while the
 * stream is being captured). Runs on the context's first device. */
int vrt_render_rows_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                          int32_t row0, int32_t rows, int32_t row_step,
                          float* d_out_rgba, vrt_hit* d_out_hit, uint64_t* d_counters,
                          void* hip_stream);

/* Pitched form (ABI v4): output row i starts i*pitch pixels after d_out_rgba (pitch >= width),
 * so a band can be written straight into its rows of a whole frame: d_out = frame + row0*width,
 * pitch = row_step*width. vrt_render_rows_async is this with pitch = width. */
int vrt_render_rows_pitched_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                                  int32_t row0, int32_t rows, int32_t row_step, int64_t pitch,
                                  float* d_out_rgba, vrt_hit* d_out_hit, uint64_t* d_counters,
                                  void* hip_stream);

/* ---- ray queries (added within v15: detect by symbol lookup) -------------------------------- */
/* Batched ray casts and pixel picks on the resident volume, without rendering a frame: which voxel,
 * and which of its faces, a ray or the cursor meets (the question an editor asks before
 * vrt_update_volume_region), whether a segment hits anything, whether a point sees another. One ray
 * per GPU lane through the frame kernels' own exact walks (RayMarch / RayMarchShadow, voxel.glsl:
 * 302-384 / :259-300), so every field below is bit-exact against the CPU oracle's march of the same
 * ray. Queries run on the context's first device. */

/* 32 bytes, 16-byte aligned in device buffers. Volume coordinates: the shader's ray.pos, i.e.
 * world + N/2 (voxel.glsl:430); the volume is [0, N]^3. dir is used as given (RayMarch does not
 * normalise it; ray_length is the parameter along dir, a distance when |dir| = 1). */
typedef struct { float origin[3]; float max_length; float dir[3]; uint32_t reserved; } vrt_ray;

/* 32 bytes. The first 16 bytes are a vrt_hit. */
typedef struct {
  int32_t voxel_index;   /* texel GetVoxel read (canonical, REPEAT wrap as vrt_hit), -1 = none */
  float ray_length;      /* RayIntersection.rayLength, 0 if none */
  uint32_t steps;        /* iterations of this one march */
  uint32_t flags;        /* VRT_HIT_FLAG_TIE3 | VRT_HIT_FLAG_STEP_CAP | VRT_RAY_FLAG_BLOCKED */
  float point[3];        /* RayIntersection.point, 0 if none */
  uint32_t face;         /* bits 0-1: axis (intersectionAxis row, tie 3 clamped to 2); bit 2: the
                            normal -sign(dir[axis]) is negative; bits 8-15: the voxel byte */
} vrt_ray_hit;

#define VRT_RAY_FLAG_BLOCKED 8u
enum { VRT_CAST_NEAREST = 0, VRT_CAST_OCCLUSION = 1 };

/* `count` rays from the DEVICE buffer d_rays into the DEVICE buffer d_hits (both 16-byte aligned, on
 * the context's first device), enqueued on `hip_stream` (hipStream_t, NULL = default): no host
 * synchronisation, no allocation. Ordering against edits and uploads on a caller stream is the
 * caller's, as for vrt_render_rows_async.
 *   VRT_CAST_NEAREST: RayMarch of a ray in air from ray length 0, ended at the ray's max_length (the
 *     loop-top test `rayLength < max_length`, voxel.glsl:317, so the step that starts below it still
 *     lands). The first non-empty voxel is the hit, glass included. A miss writes voxel_index = -1
 *     and zeros elsewhere; steps and flags are kept.
 *   VRT_CAST_OCCLUSION: RayMarchShadow along dir, in which glass does not block. Writes voxel_index =
 *     -1, ray_length = 0, point = 0, face = 0; steps and the TIE3 / STEP_CAP flags come from the walk,
 *     and VRT_RAY_FLAG_BLOCKED is set when an opaque voxel is met before max_length.
 * Nothing on the device validates a ray: a direction with a zero, tiny (below 2^-64), huge (above
 * 1e4) or non-finite component gets whatever the literal replay of the shader's loop produces (e.g.
 * an all-zero direction ends after one step, NaN lengths end at once), bounded by VRT_MAX_STEPS
 * (VRT_HIT_FLAG_STEP_CAP); every load stays inside the volume.
 * VRT_ERR_NO_VOLUME without a resident volume; VRT_ERR_INVALID for count < 0 or > 2^30, an unknown
 * mode, a null or not 16-byte aligned pointer with count > 0. count == 0 is a successful no-op. */
int vrt_cast_rays_async(vrt_ctx* ctx, const vrt_ray* d_rays, int64_t count, int32_t mode,
                        vrt_ray_hit* d_hits, void* hip_stream);

/* The same from and to HOST buffers, synchronous, through context-owned device staging that grows
 * on demand (freed by vrt_destroy). Runs on a context stream, after any preceding
 * vrt_update_volume_region (which returns only when the edit is complete). */
int vrt_cast_rays(vrt_ctx* ctx, const vrt_ray* rays, int64_t count, int32_t mode, vrt_ray_hit* hits);

/* Pixel picks (HOST buffers, synchronous): `pixels` holds `count` pairs {px, py}, py = frame row,
 * 0 = bottom. The kernel builds each pixel's primary ray exactly as a frame of (cam, params) does
 * (vertex stage at the pixel centre, RandomizeDirection at params->ray_noise and params->time) and
 * marches it in VRT_CAST_NEAREST mode with params->max_ray_length, so the first 8 bytes of a record
 * equal the vrt_hit that vrt_render writes for that pixel; point and face are what an editor needs
 * (the face's neighbour cell is where a placed block goes). Only those params fields are read.
 * VRT_ERR_INVALID for a pixel outside the image, null pointers with count > 0 or count < 0. */
int vrt_pick_pixels(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                    const int32_t* pixels, int32_t count, vrt_ray_hit* hits);

/* ---- shaded ray queries (added within v15: detect by symbol lookup) -------------------------- */
/* What a ray SEES: fragment main (voxel.glsl:425-452) for a list of rays or of pixels, without a
 * frame: other camera models (panorama, cube map, orthographic, stereo, lens jitter, supersampling;
 * vrt.panorama_rays of the Python host is a worked example), re-shading a sparse set of pixels after
 * an edit, the colour along an arbitrary world ray. One ray tree per GPU lane through the frame
 * kernels' own exact path (TraceWithShadow, the bounce stack, the colour folded in the reference's
 * order) with exact walks only, never certified walks: a record is the shader's for every input,
 * hit fields bit-exact and colour within the frame's tolerance against the CPU oracle. Traces run on
 * the context's first device. */

/* 32 bytes. The first 16 bytes are a vrt_hit of the ray's tree, as vrt_render writes per pixel. */
typedef struct {
  int32_t voxel_index;  /* the FIRST march's hit texel, -1 = none */
  float ray_length;     /* its RayIntersection.rayLength, 0 if none */
  uint32_t steps;       /* DDA + shadow-DDA iterations of the whole tree */
  uint32_t flags;       /* VRT_HIT_FLAG_TIE3 | STEP_CAP | STACK_FULL */
  float rgba[4];        /* f_Color: the folded colour, a = 1 (voxel.glsl:451) */
} vrt_ray_color;

/* `count` rays from the DEVICE buffer d_rays into the DEVICE buffer d_out (both 16-byte aligned, on
 * the context's first device), enqueued on `hip_stream` (hipStream_t, NULL = default): no host
 * synchronisation, no allocation, capturable like vrt_cast_rays_async; one launch per call. Ordering
 * against edits and uploads on a caller stream is the caller's.
 * Each ray runs main with stack[0] = Ray(origin, dir, 0, 1.0, air, 0, 0):
 *   - origin and dir are in volume coordinates (vrt_ray) and used as given: no RandomizeDirection on
 *     the first ray, so params->ray_noise is not read, and dir is not normalised, as in vrt_cast_rays;
 *   - the ray's own max_length plays u_MaxRayLength for the whole tree: secondary rays inherit the
 *     accumulated length and shadow rays get what is left, exactly as in a frame;
 *     params->max_ray_length is not read;
 *   - sun_dir, time, reflection_noise and refraction_noise, max_reflections and max_transparencies,
 *     color_only and the atlas fields are the frame's; textured mode (color_only = 0) uses the
 *     context's atlas by the render calls' rule (vrt_upload_atlas).
 * Nothing on the device validates a ray: a direction with a zero, tiny (below 2^-64), huge (above
 * 1e4) or non-finite component gets whatever the literal replay of the shader's loops produces,
 * bounded by VRT_MAX_STEPS per march (VRT_HIT_FLAG_STEP_CAP); every load stays inside the volume.
 * VRT_ERR_NO_VOLUME without a resident volume; VRT_ERR_INVALID for count < 0 or > 2^30, null params,
 * a null or not 16-byte aligned pointer with count > 0, max_reflections or max_transparencies outside
 * 0..8, and textured mode without a matching atlas (the render calls' rule). count == 0 is a
 * successful no-op. A failed call writes nothing. */
int vrt_trace_rays_async(vrt_ctx* ctx, const vrt_ray* d_rays, int64_t count, const vrt_params* params,
                         vrt_ray_color* d_out, void* hip_stream);

/* The same from and to HOST buffers, synchronous, through the ray queries' device staging (records are
 * 32 bytes either way). Runs on a context stream, after any preceding vrt_update_volume_region. */
int vrt_trace_rays(vrt_ctx* ctx, const vrt_ray* rays, int64_t count, const vrt_params* params,
                   vrt_ray_color* out);

/* Shaded pixels (HOST buffers, synchronous): `pixels` holds `count` pairs {px, py}, py = frame row,
 * 0 = bottom. The kernel builds each pixel's primary ray exactly as a frame of (cam, params) does
 * (vertex stage at the pixel centre, RandomizeDirection at params->ray_noise and params->time) and
 * traces it with params->max_ray_length: the record's first 16 bytes equal the vrt_hit that
 * vrt_render writes for that pixel, and rgba equals its float colour, bit for bit.
 * VRT_ERR_INVALID also for a null camera, a bad image size or a pixel outside the image. */
int vrt_trace_pixels(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                     const int32_t* pixels, int32_t count, vrt_ray_color* out);

/* ---- ID and depth pass (added within v15: detect by symbol lookup) --------------------------- */
/* What the frame SHOWS, per pixel and without shading: the voxel and the face the pixel's primary ray
 * meets, and the hit's depth. An ID buffer outlines a selection, an edited box or the voxels under the
 * cursor without a pick per pixel; a depth buffer composites rasterised gizmos, particles or UI against
 * the ray-traced frame; face and voxel byte per pixel guide an edge-aware filter. By default every pixel is
 * walked by the pick's exact march, an 8x8 tile per wave, in one kernel launch: the price of vrt_pick_pixels
 * over every pixel without its pixel list, its 32-byte records and its host staging. With
 * vrt_set_ids_certified(1) on an octant layout the launch is the certified ID kernel instead: the same tiles,
 * each pixel by the certified walk, and a pixel that walk cannot settle by the exact march in its own lane of
 * the same kernel; the records and depths are the same bytes (DESIGN.md §6 "ID and depth pass"). The pass
 * runs on the context's first device. */

/* 8 bytes. voxel_index and face are vrt_ray_hit's fields of the same names for the pixel's primary ray
 * (a miss: voxel_index = -1, face = 0). */
typedef struct { int32_t voxel_index; uint32_t face; } vrt_pixel_id;

/* Rows [row0, row0 + rows) of the frame of (cam, params), pixel (px, row0 + i) at d_ids[i * pitch + px]
 * (and d_depth likewise; d_depth may be NULL). DEVICE buffers on the context's first device, enqueued on
 * hip_stream (hipStream_t, NULL = default), no host synchronisation.
 * The primary ray is the frame's own (vertex stage at the pixel centre, RandomizeDirection at
 * params->ray_noise and params->time), marched in VRT_CAST_NEAREST mode with params->max_ray_length:
 * voxel_index and face equal vrt_pick_pixels' record of the pixel bit for bit, glass included. Only the
 * params fields the pick reads are read.
 * depth: with a the face's axis (face & 3) and `plane` the integer coordinate of the hit face along a,
 * depth = (float(plane) - pos[a]) / dir[a] in float32 (one subtraction, one correctly rounded division),
 * +INFINITY for a miss. It is the parameter along the NORMALISED primary direction from pos, the pixel's
 * point on the near plane in volume coordinates (world + N/2), i.e. the Euclidean distance from that
 * point to the hit, not from the eye and not a projected z. A caller that composites against a rasteriser
 * converts it: the hit point is pos + depth * dir with pos and dir from the camera's inverse matrix as the
 * vertex stage forms them (pos = near-plane point of the pixel centre, dir = normalize(far - near)); the
 * distance from the eye adds |pos - eye| (the near-plane distance over the cosine of the pixel's angle to
 * the view axis), and view-space z is (distance from the eye) times that cosine. depth is defined by the
 * face's plane; it is NOT the shader's accumulated rayLength (vrt_ray_hit::ray_length), from which it
 * differs by that sum's rounding.
 * One call is one kernel launch (one launch for vrt_set_launch_timing): no allocation, no memset, no
 * context-owned state, so calls on different streams do not disturb each other and a call is capturable in
 * a hipGraph like vrt_render_rows_async.
 * VRT_ERR_NO_VOLUME without a resident volume; VRT_ERR_INVALID for a null cam, params or d_ids, a bad image
 * size, rows < 0 or a band outside the image, pitch < width, d_ids not 8-byte or d_depth not 4-byte
 * aligned. rows == 0 is a successful no-op. A failed call writes nothing. */
int vrt_render_ids_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params, int32_t row0,
                         int32_t rows, int32_t pitch, vrt_pixel_id* d_ids, float* d_depth, void* hip_stream);

/* Whole frame to HOST buffers (width * height records, row 0 = bottom; depth may be NULL), synchronous,
 * through context-owned device staging that grows on demand. Runs on a context stream, after any
 * preceding vrt_update_volume_region. */
int vrt_render_ids(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params, vrt_pixel_id* ids,
                   float* depth);

/* Of the last synchronous vrt_render_ids: pixels rendered, and how many of them were walked by the exact
 * march: all of them when the exact ID kernel ran (mode 0, or the single layout); with the certified ID
 * kernel, the pixels its walk left to the exact march in their lanes (counted through a context-owned device
 * word that only the synchronous call zeroes, passes and reads back). Zeros before the first such call. */
int vrt_ids_deferred(vrt_ctx* ctx, uint64_t* pixels, uint64_t* deferred);

/* The ID pass's kernel (added within v15: detect by symbol lookup). mode 0 (the default): the exact ID kernel
 * for every pixel. mode 1: the certified ID kernel where the resident volume has the eight-octant skip layout
 * (vrt_volume_octants() == 8); on the single layout (N = 1024, vrt_set_skip_layout(1)) the exact kernel still
 * runs. One kernel and one launch either way: a pixel whose certified walk is unsure, or whose start the
 * walk's checks refuse, is walked exactly in its own lane, so vrt_render_ids_async keeps its contract (no
 * allocation, no memset, no atomics, no context-owned state, capturable) and vrt_render_ids,
 * vrt_render_ids_async and vrt_render_frame_reprojected return the same bytes in both modes. The mode
 * survives uploads. VRT_ERR_INVALID for any other mode (nothing changes) or a null context. */
int vrt_set_ids_certified(vrt_ctx* ctx, int32_t mode);

/* 1 when the next ID pass will launch the certified ID kernel (mode 1 and an octant layout resident), else 0. */
int vrt_ids_certified(const vrt_ctx* ctx);

/* ---- reprojected temporal filter (added within v15: detect by symbol lookup) ----------------- */
/* A temporal filter whose history follows the camera: the first consumer of the ID and depth pass. The
 * reference's filter (temporal.glsl:18, vrt_render_frame) blends a pixel with the same pixel of the previous
 * filtered frame, which is right only while the camera stands still. Here each pixel's history is fetched
 * where its surface point was on screen in the previous frame, and it is used only if the previous frame
 * showed the same face of the same voxel with the same material byte there: both words of the two
 * vrt_pixel_id records equal, no depth or normal threshold. An edited voxel drops its history by
 * construction (DESIGN.md §6 "Reprojected temporal filter"). */

/* The filter over rows [row0, row0 + rows) of the current frame, one kernel launch on hip_stream (one
 * launch for vrt_set_launch_timing), on the context's first device: no memset, no allocation, no atomics, no
 * context-owned state, capturable like vrt_render_ids_async.
 *   d_raw_rgba8, d_ids, d_depth, d_out_rgba8, d_src (optional): band-indexed, pixel (px, row0 + i) at
 *     [i * pitch + px], as vrt_render_ids_async writes d_ids and d_depth. d_raw_rgba8 is the quantised
 *     ray-traced frame (RGBA8 words, e.g. vrt_render_temporal_rows_async at u_Alpha = 1).
 *   d_prev_rgba8, d_prev_ids: the WHOLE previous filtered frame and its ID records, width x height with
 *     prev_pitch >= width pixels between rows; both NULL: no history.
 *   cam, params: those d_ids and d_depth were rendered with (only the fields the pick reads are read);
 *     prev_pv: the previous frame's forward matrix (vrt_camera_forward of its camera).
 * Per pixel, in float32 and in exactly this order (no contraction, correctly rounded division):
 *   1. pos, dir: the pixel's primary ray, as vrt_render_ids_async forms it (depth is measured along it);
 *   2. a hit (voxel_index >= 0): v[i] = (pos[i] + depth * dir[i]) - float(N) * 0.5f, w = 1;
 *      a miss: v = dir, w = 0 (the sky is a point at infinity);
 *   3. clip[r] = ((m[0*4+r] * v.x + m[1*4+r] * v.y) + m[2*4+r] * v.z) + m[3*4+r] * w, m = prev_pv;
 *   4. !(clip[3] > 0): code -2 (behind the previous camera, or NaN);
 *   5. sx = ((clip[0] / clip[3]) * 0.5f + 0.5f) * float(width), sy likewise from clip[1] and height;
 *   6. !(sx >= 0 && sx < width && sy >= 0 && sy < height), on the floats: code -1;
 *   7. qx = int(floorf(sx)), qy = int(floorf(sy)): a nearest fetch;
 *   8. either word of d_prev_ids[qy * prev_pitch + qx] differs from the pixel's d_ids record: code -3;
 *   9. else accepted: src = qy * width + qx.
 * Accepted pixels get temporal.glsl's blend of the raw pixel with d_prev_rgba8[qy * prev_pitch + qx] at
 * alpha (the frame kernels' own blend on RGB8 texels), every other pixel the raw pixel. d_src receives src
 * or the code; -4 = no history (precedence -4, -2, -1, -3).
 * The output must not alias the previous frame (the kernel reads other pixels' history).
 * VRT_ERR_NO_VOLUME without a resident volume; VRT_ERR_INVALID for a null cam, params, prev_pv, d_raw_rgba8,
 * d_ids, d_depth or d_out_rgba8, a bad image size, rows < 0 or a band outside the image, pitch or prev_pitch
 * < width, exactly one of d_prev_rgba8 and d_prev_ids NULL, d_out_rgba8 == d_prev_rgba8, an ID buffer not
 * 8-byte or another buffer not 4-byte aligned. rows == 0 is a successful no-op. A failed call writes nothing. */
int vrt_reproject_temporal_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                                 const float prev_pv[16], float alpha, int32_t row0, int32_t rows, int32_t pitch,
                                 const uint32_t* d_raw_rgba8, const vrt_pixel_id* d_ids, const float* d_depth,
                                 const uint32_t* d_prev_rgba8, const vrt_pixel_id* d_prev_ids, int32_t prev_pitch,
                                 uint32_t* d_out_rgba8, int32_t* d_src, void* hip_stream);

/* The synchronous frame loop with that filter: like vrt_render_frame, with a history of its own in the
 * context (ping-pong filtered frames and ID buffers, the previous camera's forward matrix, staging that
 * grows on demand; vrt_render_frame's history is not touched). Each call, on a context stream of the first
 * device (multi-device contexts run all of it there, like the ID pass): the quantised ray-traced frame of
 * (cam, params); the ID and depth pass of (cam, params with ray_noise = 0): geometry buffers are noise-free,
 * since a noised primary ray's hit belongs at another screen position; the filter with those noise-free
 * params against the previous call's output, IDs and matrix; the copy to out_rgba8 (W*H*4 bytes).
 * The first call has no history, so its output is the raw frame, as is the first after a change of the image
 * size, after vrt_reprojected_history_reset, or after a frame whose camera matrix has no inverse.
 * stats (optional): kernel_ms is the GPU time from the first launch's start to the last launch's end;
 * counters (VRT_STATS_COUNTERS) are VRT_ERR_UNSUPPORTED.
 * Limits: the default fetch is nearest, so a history that is resampled frame after frame drifts by up to
 * half a pixel per frame (vrt_set_reprojected_fetch selects the bilinear fetch); the ID pass runs inside
 * every call (the exact ID kernel, or the certified one after vrt_set_ids_certified(1): the same bytes). */
int vrt_render_frame_reprojected(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params, float alpha,
                                 uint8_t* out_rgba8, vrt_stats* stats);

/* The next vrt_render_frame_reprojected has no history: its output is its raw frame. */
int vrt_reprojected_history_reset(vrt_ctx* ctx);

/* ---- bilinear history fetch (added within v15: detect by symbol lookup) ----------------------- */
/* The history fetch of the reprojected filter as a mode. VRT_FETCH_NEAREST is the filter above.
 * VRT_FETCH_BILINEAR fetches the four texels around the reprojected position and keeps those that show the
 * pixel's own voxel face: a history resampled frame after frame no longer jitters by half a pixel, and a
 * pixel whose nearest texel shows another face keeps the history of its neighbours that do not. */
enum { VRT_FETCH_NEAREST = 0, VRT_FETCH_BILINEAR = 1 };

/* vrt_reproject_temporal_async with a fetch mode and an optional tap mask. Everything said there about the
 * arguments holds here: band indexing, the pitches, the aliasing rule, the errors, rows == 0 as a successful
 * no-op, a failed call writes nothing; one kernel launch on hip_stream (one launch for vrt_set_launch_timing),
 * no memset, no allocation, no atomics, no context-owned state, capturable. In addition an unknown fetch is
 * VRT_ERR_INVALID, and d_taps (optional) is one byte per pixel at [i * pitch + px], of any alignment.
 * VRT_FETCH_NEAREST: d_out_rgba8 and d_src are vrt_reproject_temporal_async's bytes (without d_taps it is
 * the same kernel); d_taps is 1 for an accepted pixel, else 0.
 * VRT_FETCH_BILINEAR, per pixel, in float32 and in exactly this order (no contraction, correctly rounded
 * division): steps 1-6 above, which give sx, sy and the codes -4, -2 and -1 with the same precedence; then
 *   7. tx = sx - 0.5f, x0 = floorf(tx), fx = tx - x0, ix0 = int(x0); ty, y0, fy, iy0 likewise (texel centres
 *      sit at +0.5; ix0 may be -1 and ix0 + 1 may be width, rows likewise);
 *   8. tap k = 0..3 at (ix0 + (k & 1), iy0 + (k >> 1)), with the weights w0 = (1 - fx) * (1 - fy),
 *      w1 = fx * (1 - fy), w2 = (1 - fx) * fy, w3 = fx * fy;
 *   9. tap k is valid iff its coordinates lie in [0, width) x [0, height), w_k > 0, and both words of
 *      d_prev_ids there equal the pixel's d_ids record; a tap outside the previous image is never loaded;
 *  10. wsum = ((v0 + v1) + v2) + v3 with v_k = valid ? w_k : 0; no valid tap: code -3, the raw pixel;
 *  11. else accepted; per channel, with c_k the tap's byte / 255 (correctly rounded):
 *      h = (((v0 * c0 + v1 * c1) + v2 * c2) + v3 * c3) / wsum,
 *      out = unorm8(alpha * (raw byte / 255) + (1.0f - alpha) * h), A = 255: the history is filtered once
 *      and the colour quantised once;
 *  12. d_src = qy * width + qx with (qx, qy) = floor(sx, sy), the nearest texel, which is one of the four
 *      taps (valid or not); d_taps = the mask of valid taps, bit k for tap k, 0 for a pixel not accepted.
 * With an unmoved camera this mode is NOT byte-equal to vrt_render_frame's filter: the float round trip leaves
 * fx and fy within about 1e-3 of 0 or 1, so the neighbours enter with tiny weights. */
int vrt_reproject_temporal_fetch_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                                       const float prev_pv[16], float alpha, int32_t fetch, int32_t row0,
                                       int32_t rows, int32_t pitch, const uint32_t* d_raw_rgba8,
                                       const vrt_pixel_id* d_ids, const float* d_depth,
                                       const uint32_t* d_prev_rgba8, const vrt_pixel_id* d_prev_ids,
                                       int32_t prev_pitch, uint32_t* d_out_rgba8, int32_t* d_src, uint8_t* d_taps,
                                       void* hip_stream);

/* The fetch mode of vrt_render_frame_reprojected's filter; VRT_FETCH_NEAREST in a new context. The history
 * (frames, IDs, matrix) is kept across a switch. An unknown mode is VRT_ERR_INVALID and changes nothing. */
int vrt_set_reprojected_fetch(vrt_ctx* ctx, int32_t fetch);

/* ---- ID-guided spatial filter (added within v15: detect by symbol lookup) --------------------- */
/* The edge-aware filter the ID pass guides: an edge-stopping à-trous filter on RGBA8 frames whose edge stop
 * is the ID record itself. A pixel that has just lost its history (a disoccluded pixel, an edited voxel, the
 * first frame after a reset) shows its raw, noisy sample; this filter gives it the mean of its neighbours on
 * the same surface. It follows the reprojected filter's rule: a tap counts only if it shows the same surface,
 * words compared for equality, with no depth or normal threshold. All integer arithmetic
 * (DESIGN.md §6 "Spatial filter"). */
enum { VRT_GUIDE_FACE = 0, VRT_GUIDE_PLANE = 1 };

/* One à-trous pass over rows [row0, row0 + rows) of a width x height frame: one kernel launch on hip_stream
 * (one launch for vrt_set_launch_timing), on the context's first device: no memset, no allocation, no atomics,
 * no context-owned state, capturable like vrt_render_ids_async.
 * All buffers are DEVICE buffers indexed by the WHOLE frame: pixel (x, y) at [y * pitch + x]. d_in_rgba8 and
 * d_out_rgba8 hold RGBA8 words, d_ids the frame's vrt_pixel_id records; d_keep and d_count (both optional)
 * hold one byte per pixel and may have any alignment. The call writes rows [row0, row0 + rows) of d_out_rgba8
 * and d_count and nothing else; it reads taps from the whole image, so d_out_rgba8 must not alias d_in_rgba8.
 * Per pixel P = (x, y) of the band, in integers:
 *   1. d_keep given and d_keep[P] != 0: out[P] = in[P], all four bytes, count[P] = 0. (A kept pixel still
 *      serves as a tap of other pixels.)
 *   2. tap (i, j), i, j in -2..2, sits at T = (x + i * step, y + j * step) with the weight K[i+2] * K[j+2],
 *      K = {1, 4, 6, 4, 1};
 *   3. T is valid iff it lies in [0, width) x [0, height), key(T) == key(P), and |dR| + |dG| + |dB| <= range
 *      between in[T] and in[P] (the A bytes are ignored). A tap outside the image is never loaded, neither its
 *      ID nor its colour. The centre is always valid;
 *   4. key, VRT_GUIDE_FACE: both words of the record. (The ID pass writes every miss as {-1, 0}: all misses
 *      share one key.)
 *      key, VRT_GUIDE_PLANE: the face word, and for a hit (voxel_index >= 0) the cell coordinate along the
 *      face's axis, (voxel_index >> ((face & 3) * log2 N)) & (N - 1) with N the resident volume's edge, in
 *      place of the voxel index; a miss keeps its negative word. Coplanar faces of one material and one
 *      orientation filter together. PLANE is meant for opaque surfaces: glass shows view-dependent content
 *      across a plane;
 *   5. wsum = the sum of the valid weights (36..256), acc_c = the sum of weight * byte_c over the valid taps;
 *      out_c = (2 * acc_c + wsum) / (2 * wsum), integer floor, for c = R, G, B; A = 255;
 *      count[P] = the number of valid taps, 1..25.
 * VRT_ERR_NO_VOLUME without a resident volume (both guides). VRT_ERR_INVALID for a null d_in_rgba8, d_ids or
 * d_out_rgba8, a bad image size (vrt_render_ids_async's rule), pitch < width, rows < 0 or a band outside the
 * image, step outside 1..64, an unknown guide, range < 0 (765 or more disables the colour test),
 * d_out_rgba8 == d_in_rgba8, d_ids not 8-byte or a colour buffer not 4-byte aligned. rows == 0 is a successful
 * no-op. A failed call writes nothing. */
int vrt_spatial_filter_async(vrt_ctx* ctx, int32_t width, int32_t height, int32_t pitch, int32_t step,
                             int32_t guide, int32_t range, int32_t row0, int32_t rows,
                             const uint32_t* d_in_rgba8, const vrt_pixel_id* d_ids, const uint8_t* d_keep,
                             uint32_t* d_out_rgba8, uint8_t* d_count, void* hip_stream);

/* `passes` passes (1..5) over HOST buffers of packed width x height, pass p = 0, 1, ... at step 2^p, each the
 * pass above over the whole frame with the same ids, keep (optional), guide and range; synchronous, through
 * context-owned device staging that grows on demand and is freed by vrt_destroy, on the main context stream
 * of the first device. Errors as above; also VRT_ERR_INVALID for passes outside 1..5. */
int vrt_spatial_filter(vrt_ctx* ctx, int32_t width, int32_t height, int32_t passes, int32_t guide, int32_t range,
                       const uint8_t* rgba8, const vrt_pixel_id* ids, const uint8_t* keep, uint8_t* out_rgba8);

/* The spatial passes of vrt_render_frame_reprojected; VRT_SPATIAL_OFF in a new context (the loop then runs
 * exactly the launches described there). The passes run after the temporal filter, pass p at step 2^p, on the
 * frame's noise-free IDs.
 *   VRT_SPATIAL_DISPLAY: the returned frame is the passes applied to the temporal filter's output, without a
 *     keep mask; the history stays the unfiltered temporal output, so the history chain is that of a context
 *     with the passes off.
 *   VRT_SPATIAL_FILL: the passes run with d_keep = the temporal filter's tap byte (the loop launches the fetch
 *     with a tap buffer): a pixel with accepted history is kept, a pixel without gets its spatial estimate.
 *     The filled frame is the returned frame and the next call's history.
 * stats->kernel_ms spans to the last pass's end. The history (frames, IDs, matrix) is kept across a switch.
 * An unknown mode or guide, passes outside 1..5 or range < 0 is VRT_ERR_INVALID and changes nothing. */
enum { VRT_SPATIAL_OFF = 0, VRT_SPATIAL_DISPLAY = 1, VRT_SPATIAL_FILL = 2 };
int vrt_set_reprojected_spatial(vrt_ctx* ctx, int32_t mode, int32_t passes, int32_t guide, int32_t range);

/* ---- textured mode (voxel.glsl without _COLOR_ONLY) --------------------- */
/* With vrt_params.color_only = 0 the kernel shades with the textured material table
 * (voxel.glsl:51-68) and GetColor reads the atlas (:174-182) at GetTextureCoordinate (:167-172)
 * of the hit's face plane, with atlas_size = u_AtlasSize and atlas_texture_size =
 * u_AtlasTextureSize (main.cpp:336-337). Atlas: atlas_size^2 RGBA8 texels, row 0 = bottom (GL
 * t = 0), NEAREST + REPEAT; material slot (texX, texY) covers columns [texX*ts, (texX+1)*ts) and
 * rows [size-(texY+1)*ts, size-texY*ts). atlas_size must be a power of two. The context keeps
 * the atlas: it is uploaded by vrt_upload_atlas, or by any render call whose
 * vrt_params.atlas_rgba is non-NULL and whose bytes (or size) differ from the last upload
 * (compared on the host each call; a synchronous copy when they differ; ABI v8: by content, not
 * by pointer identity). atlas_rgba = NULL renders with the context's atlas: a frame loop uploads
 * once and passes NULL (a non-NULL atlas costs a host compare of its bytes on every call, ~10 us
 * for 256 x 256). Replaces the Atlas texture of main.cpp:187-193. */
int vrt_upload_atlas(vrt_ctx* ctx, const uint8_t* rgba, int32_t atlas_size);

/* ---- temporal filter + RGB8 framebuffer ------------------------------ */
/* The reference stores the ray-traced colour into an RGB8 FBO (FrameBuffer.cpp:8), blends it with
 * the previous filtered frame, color = u_Alpha * new + (1 - u_Alpha) * old (temporal.glsl:18,
 * main.cpp:363-377), into a second RGB8 FBO and swaps the two (main.cpp:391). These entry points
 * run that post-pass fused into the render kernel's epilogue. Pixels are RGBA8 words (R in the
 * low byte, A = 255: the FBOs have no alpha), W x rows, row 0 = bottom. Float -> UNORM8 store:
 * clamp [0,1], x255, round half to even, NaN -> 0 (GL leaves ties/NaN implementation-defined).
 * u_Alpha defaults to 1.0 (res/guis/header.xml:20), which makes the output the quantised frame. */

/* Asynchronous band form on DEVICE buffers, same band/counter/stream rules as
 * vrt_render_rows_async. d_prev_rgba8 holds the band's previous filtered frame and may alias
 * d_cur_rgba8 (each pixel is read before it is written, by the same work-item). d_raw_rgba8
 * (optional) receives the quantised ray-trace frame. */
int vrt_render_temporal_rows_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                                   float alpha, int32_t row0, int32_t rows, int32_t row_step,
                                   const uint32_t* d_prev_rgba8, uint32_t* d_cur_rgba8,
                                   uint32_t* d_raw_rgba8, vrt_hit* d_out_hit, uint64_t* d_counters,
                                   void* hip_stream);

/* Pitched form (ABI v4): row i of d_prev_rgba8, d_cur_rgba8, d_raw_rgba8 and d_out_hit starts
 * i*pitch pixels after the pointer (pitch >= width). With d_prev = d_cur = frame + row0*width and
 * pitch = row_step*width a band filters its rows of one full-frame history in place — the
 * single-GPU frame loop needs no per-band buffers and no assembly copy. */
int vrt_render_temporal_rows_pitched_async(vrt_ctx* ctx, const vrt_camera* cam,
                                           const vrt_params* params, float alpha, int32_t row0,
                                           int32_t rows, int32_t row_step, int64_t pitch,
                                           const uint32_t* d_prev_rgba8, uint32_t* d_cur_rgba8,
                                           uint32_t* d_raw_rgba8, vrt_hit* d_out_hit,
                                           uint64_t* d_counters, void* hip_stream);

/* ABI v11: block-cyclic bands. Band row i is frame row
 *   row0 + (i / row_block) * row_step + i % row_block
 * i.e. blocks of row_block adjacent frame rows, row_step frame rows apart (GPU r of a k-way split
 * with blocks of B rows: row0 = r*B, row_step = k*B, rows = its blocks' rows). row_block is a
 * power of two in [1, 64], and row_step >= row_block unless rows <= row_block; row_block = 1 is the
 * cyclic-row form above. With row_block = 8 an 8x8 pixel wave covers 8 adjacent frame rows, as in
 * a whole frame, instead of 8 rows k apart: the walks of a wave's rays stay coherent (one-GPU
 * rehearsal of GPU 0's band at k = 8: C4 -7 %, C3 -11 % per frame). Everything else
 * (pitch, history, counters, stream, timing) as vrt_render_rows_pitched_async and
 * vrt_render_temporal_rows_pitched_async. */
int vrt_render_blocks_pitched_async(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                                    int32_t row0, int32_t rows, int32_t row_step, int32_t row_block,
                                    int64_t pitch, float* d_out_rgba, vrt_hit* d_out_hit,
                                    uint64_t* d_counters, void* hip_stream);
int vrt_render_temporal_blocks_pitched_async(vrt_ctx* ctx, const vrt_camera* cam,
                                             const vrt_params* params, float alpha, int32_t row0,
                                             int32_t rows, int32_t row_step, int32_t row_block,
                                             int64_t pitch, const uint32_t* d_prev_rgba8,
                                             uint32_t* d_cur_rgba8, uint32_t* d_raw_rgba8,
                                             vrt_hit* d_out_hit, uint64_t* d_counters,
                                             void* hip_stream);

/* ABI v14: a FRAME BATCH: the same band of `nframes` (1..8) frames in ONE launch, at u_Alpha = 1
 * (each frame's RGB8 store is its output; no history is read), frame f with its own camera
 * cams[f] (same image size) and u_Time params[f].time, written to d_cur_rgba8[f] (and
 * d_raw_rgba8[f] when d_raw_rgba8 is not NULL; pitch
 * pixels per band row in all of them). Band geometry as vrt_render_temporal_blocks_pitched_async;
 * bands of < 8192 rows. A band of a k-way split is 1/k of the frame's waves: below a few dispatch
 * rounds a launch is bound by its longest waves and by the hardware queues that overlap launches,
 * not by the GPU's throughput, and a batch of k frames gives it a whole frame's waves again (the
 * deferred exact pass, the tile order and the grid sizing then see one large launch). Bytes equal
 * nframes single-frame launches' (tests/test_gpu_batch.py). No hit records or counters. A batch
 * of more than 131072 tiles (16x8 pixels) is enqueued as the fewest launches that hold it, of
 * equal frame counts. ABI v15: consecutive frames whose other params fields differ (the day/night
 * cycle moves u_SunDir every frame, main.cpp:346-348) are split into launches of equal fields, in
 * frame order on the stream (before v15: an error). */
int vrt_render_temporal_batch_async(vrt_ctx* ctx, int32_t nframes, const vrt_camera* cams,
                                    const vrt_params* params, int32_t row0, int32_t rows,
                                    int32_t row_step, int32_t row_block, int64_t pitch,
                                    uint32_t* const* d_cur_rgba8, uint32_t* const* d_raw_rgba8,
                                    void* hip_stream);

/* Synchronous frame loop of main.cpp:323-393 with the history and the ray-trace FBO kept in the
 * context: render, filter against the last filtered frame, copy the new filtered frame to the
 * HOST buffer out_rgba8 (W*H*4 bytes). The history starts black and restarts black when the image
 * size changes. stats may be NULL. Each device renders its row band as two interleaved parts on
 * two context-owned streams (one launch's tail overlaps the other's), or as one deferred launch
 * (vrt_set_exact_pass: glass-heavy volumes, large frames); ABI v9: every device's DMA
 * engine writes its band straight into its rows of a pinned staging frame owned by the context
 * (the k copies run in parallel), which is then copied to out_rgba8. */
int vrt_render_frame(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params, float alpha,
                     uint8_t* out_rgba8, vrt_stats* stats);

/* ABI v8: the same frame for display on the first device, asynchronously. *d_frame receives a
 * device pointer (first GPU) to the new filtered frame, W*H RGBA8 words, row 0 = bottom, owned by
 * the context; hip_stream is made to wait for it, so work the caller enqueues there afterwards
 * (e.g. the texture upload / blit of main.cpp:379-385) sees the frame. The frame stays valid until
 * the fourth later call, which overwrites it only after the work the caller had enqueued on
 * hip_stream before the next call. One device: the frame is rendered straight into that buffer
 * (no copy); several devices: the bands are gathered to the first one over xGMI by ncclGather
 * (rccl.h) and placed into their rows by strided copies. Consecutive frames overlap on the GPU:
 * at u_Alpha = 1 a frame does not read its history and up to four frames are in flight (ABI v9);
 * otherwise part q of a frame waits only for part q of the frame before (its history rows).
 * Returns after the launches; stats may be NULL (then no host sync happens; with stats the call
 * waits for the frame).
 * ABI v9: hip_stream = NULL orders nothing with the caller's streams. The caller then consumes the
 * frame on the stream that produced it (vrt_frame_stream, right after the call): work enqueued
 * there runs after the frame and before the frame that next reuses its buffer (the eighth later
 * call), so no ordering packet crosses streams (with a caller stream, each frame's wait costs
 * ~0.01-0.02 ms of GPU throughput at C3); the host blocks only when it is eight
 * frames ahead of the GPU. */
int vrt_render_frame_device(vrt_ctx* ctx, const vrt_camera* cam, const vrt_params* params,
                            float alpha, void* hip_stream, const uint32_t** d_frame,
                            vrt_stats* stats);

/* ABI v9: the HIP stream (hipStream_t) that rendered (or, with several devices, assembled) the last
 * device-output frame of a hip_stream = NULL call, on the first device; NULL before one. */
void* vrt_frame_stream(const vrt_ctx* ctx);

/* "Clear framebuffer" (key F, main.cpp:417-421): the last ray-traced frame becomes the history of
 * the next frame. ABI v9: no buffer changes hands (a device-output frame the caller holds keeps
 * its contents and lifetime). */
int vrt_history_reset(vrt_ctx* ctx);

/* ---- host-side scene harness (mirrors src/main.cpp; no GPU needed) ----------------------- */

enum { VRT_SCENE_TERRAIN = 0, VRT_SCENE_GLASS_CUBE = 1, VRT_SCENE_REFRACTION = 2 };

/* Build-defined seeded heightfield in [0,1) replacing Greet::Noise::GenNoise (main.cpp:185,195);
 * out has n*n floats, index x + z*n. See DESIGN.md "Terrain noise". */
int vrt_terrain_noise(int32_t n, uint32_t seed, float* out);

/* Fill out[n^3] exactly as main.cpp:218-288 does for _TERRAIN / _GLASS_CUBE / _REFRACTION. */
int vrt_build_scene(int32_t scene, int32_t n, uint32_t seed, uint8_t* out);

/* invPV = inverse(P * V) with P = Perspective(aspect, fov_deg, near, far) and
 * V = RotateX(-rot_x) * RotateY(-rot_y) * Translate(-pos)   (main.cpp:67-76, 161). Angles in
 * degrees. Computed in double, rounded to float. */
int vrt_camera_make(const float pos[3], const float rot_deg[3], int32_t width, int32_t height,
                    float fov_deg, float near_plane, float far_plane, vrt_camera* out);

/* Added within v15. PV = inverse(cam->inv_pv), column-major like inv_pv: the forward matrix that takes a
 * world point to the camera's clip coordinates (vrt_reproject_temporal_async's prev_pv). Computed in
 * double and rounded to float, as vrt_camera_make computes its inverse. Host arithmetic, no GPU.
 * VRT_ERR_INVALID for null pointers and for a singular (or non-finite) matrix. */
int vrt_camera_forward(const vrt_camera* cam, float out_pv[16]);

/* u_SunDir from the day/night clock (main.cpp:346-348). */
void vrt_sun_dir(float time_of_day, float day_time, float out[3]);

/* Default params for the bench configs (noise 0, max_ray_length 100, colour-only, time 1). */
void vrt_params_default(vrt_params* out);

/* ABI v8: the row plan of a whole frame of `height` rows over k devices with `parts` interleaved
 * parts each (host arithmetic, no GPU): for band j (device j) and part p, the frame rows
 * row0 + i*row_step (i < rows) that the part renders, written to band-buffer row
 * band_row0 + i*parts. out[(j*parts + p)*4 + 0..3] = {row0, rows, row_step, band_row0}; a band
 * holds ceil((height - j) / k) rows, band row r = frame row j + r*k. Returns the largest band's
 * rows. LEGACY (cyclic rows): since ABI v12 the whole-frame entry points split a frame of
 * k > 1 devices into block-cyclic bands (vrt_block_band_plan) and use this plan only for the
 * interleaved parts of one device's frame (k = 1); kept exported for tests. */
int vrt_band_plan(int32_t height, int32_t k, int32_t parts, int32_t* out);

/* ABI v10: the k strided copies that assemble a frame of `height` rows x `width` pixels of
 * `elem_bytes` each from the k band buffers (band j's rows packed, band row r = frame row j + r*k):
 * the pinned host staging of vrt_render / vrt_render_frame over k devices and the device-frame
 * gather use exactly these. out[j*5 + 0..4] = {destination byte offset, destination pitch, source
 * pitch, row bytes, rows} of one 2-D copy (hipMemcpy2D). Host arithmetic, no GPU; returns k.
 * LEGACY (cyclic rows, as vrt_band_plan): the k > 1 whole-frame paths use vrt_block_copy_plan's
 * copies since ABI v12. Exported for tests (unequal bands when height % k != 0). */
int vrt_band_copy_plan(int32_t width, int32_t height, int32_t k, int32_t elem_bytes, int64_t* out);

/* ABI v12: rows per block of the bands the whole-frame entry points split a frame into over k
 * devices: 1 for k = 1 (the whole frame), 16 for k > 1 (block-cyclic bands). */
int vrt_frame_row_block(int32_t k);

/* ABI v12: the block-cyclic band of every device j < k for blocks of row_block rows (a power of
 * two <= 64): out[j*3 + 0..2] = {row0, rows, row_step}, band row i = frame row
 * row0 + (i / row_block) * row_step + i % row_block (the *_blocks_pitched_async arguments; k = 1:
 * the whole frame). Returns the largest band's rows. Host arithmetic, no GPU. */
int vrt_block_band_plan(int32_t height, int32_t k, int32_t row_block, int32_t* out);

/* ABI v12: the 2-D copies that assemble a frame from k packed block-cyclic band buffers (what
 * vrt_render / vrt_render_frame stage with over k > 1 devices when row_block is
 * vrt_frame_row_block(k)): per band two entries, out[(j*2 + c)*7 + 0..6] = {band j, destination
 * byte offset, destination pitch, source byte offset, source pitch, width bytes, rows} (the band's
 * full blocks, then a short last block; rows = 0 when absent). Returns the number of copies. */
int vrt_block_copy_plan(int32_t width, int32_t height, int32_t k, int32_t row_block, int32_t elem_bytes,
                        int64_t* out);

/* ---- one process per GPU (ABI v12) ------------------------------------------------------------
 * A job of nranks processes, one GPU each (torchrun), each rendering its block-cyclic band of
 * every frame into its own buffers, gathers the bands to rank 0 over RCCL (xGMI) and assembles the
 * frame there — the drop-in's ncclGather path with the ranks in separate processes. */
#define VRT_COMM_ID_BYTES 128
/* A new RCCL unique id (ncclGetUniqueId) into out (>= VRT_COMM_ID_BYTES bytes; rank 0 creates the
 * ids and the job distributes them). Returns VRT_COMM_ID_BYTES. */
int vrt_comm_unique_id(uint8_t* out, int32_t bytes);
/* Join `count` communicators (ids: count x VRT_COMM_ID_BYTES) as `rank` of `nranks` on the
 * context's device (one-device contexts). Blocks until every rank has joined each one, in order.
 * One communicator per lane of frames in flight: a communicator's operations run in issue order,
 * separate ones do not order each other. */
int vrt_comm_join(vrt_ctx* ctx, const uint8_t* ids, int32_t count, int32_t nranks, int32_t rank);
/* ncclGather of `bytes` from d_band on every rank to rank 0's d_gathered (nranks x bytes, rank
 * order; ignored elsewhere) over communicator `comm`, enqueued on hip_stream. */
int vrt_gather_band_async(vrt_ctx* ctx, int32_t comm, const void* d_band, uint64_t bytes, void* d_gathered,
                          void* hip_stream);
/* The frame (height rows of width RGBA8 words, rows frame_pitch words apart) from k gathered
 * block-cyclic bands of row_block rows (band j at d_bands + j * band_rows_cap * width words, band
 * row i = frame row ((i / row_block) * k + j) * row_block + i % row_block): one HIP kernel, one
 * workgroup per frame row, on hip_stream. */
int vrt_assemble_blocks_async(vrt_ctx* ctx, const uint32_t* d_bands, int32_t k, int32_t band_rows_cap,
                              int32_t width, int32_t height, int32_t row_block, uint32_t* d_frame,
                              int64_t frame_pitch, void* hip_stream);
/* RGB8 wire format of a gathered band: the RGBA8 words' A byte is always 255, so a band can cross
 * xGMI as 3 bytes per pixel (25 % fewer bytes into rank 0). vrt_pack_rgb8_async packs `pixels`
 * RGBA8 words (a multiple of 4; 16-byte aligned) into 3-byte pixels (4-byte aligned);
 * vrt_assemble_blocks_rgb8_async is vrt_assemble_blocks_async from such bands (band j at
 * d_bands + j * band_rows_cap * width * 3 bytes; width and frame_pitch multiples of 4), unpacking
 * to RGBA8 words with A = 255. */
int vrt_pack_rgb8_async(vrt_ctx* ctx, const uint32_t* d_rgba8, uint64_t pixels, uint8_t* d_rgb8, void* hip_stream);
int vrt_assemble_blocks_rgb8_async(vrt_ctx* ctx, const uint8_t* d_bands, int32_t k, int32_t band_rows_cap,
                                   int32_t width, int32_t height, int32_t row_block, uint32_t* d_frame,
                                   int64_t frame_pitch, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* VRT_H */
