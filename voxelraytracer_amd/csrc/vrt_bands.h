// vrt_bands.h — the row bands of a frame over k devices, parts or ranks: which frame rows a band holds
// and the 2-D copies that place it (vrt_bands.cpp). Integer arithmetic only: no HIP, no RCCL. Not installed.
#ifndef VRT_BANDS_H
#define VRT_BANDS_H

#include <cstddef>
#include <cstdint>

// library-private: nothing here is exported
#pragma GCC visibility push(hidden)

namespace vrt {

// Whole frames over k > 1 devices (ABI v12): block-cyclic bands of kFrameRowBlock adjacent rows,
// band j = blocks j, j + k, ... (band row i = frame row ((i / B) k + j) B + i % B), one launch per
// band and frame, as bench.py's one-process-per-GPU split (tiles.block_band_spec): an 8x8 wave of
// a band covers 8 adjacent frame rows as in the whole frame, so its walks stay coherent (slowest
// of 8 bands: C3 0.0150 -> 0.0139, C4 0.0274 -> 0.0229 ms per frame against cyclic rows,
// profiles/r03_s45, r03_s54). One device renders the whole frame (B = 1, kParts parts).
constexpr int32_t kFrameRowBlock = 16;
constexpr int32_t kFrameRowBlockSh = 4;
static_assert((1 << kFrameRowBlockSh) == kFrameRowBlock, "row block is 2^sh");
struct BandGeom {
  int32_t row0, rows, row_step, sh;
};
BandGeom block_band(int32_t height, int32_t k, int32_t block, int32_t j);
int32_t largest_band(int32_t height, int32_t k, int32_t block);
int32_t frame_block(int32_t k);
int32_t band_rows(int32_t height, int32_t k, int32_t j);
int32_t band_cap(int32_t height, int32_t k);

// One 2-D copy of band_copies
struct BandCopy {
  size_t dst_off, dst_pitch, src_off, src_pitch, width, rows;
};
int band_copies(int32_t w, int32_t h, int32_t k, int32_t block, int32_t j, size_t elem, BandCopy out[2]);

// Part p of band j: frame rows (j + p k) + i (k P), band rows p + i P.
struct PartRows {
  int32_t row0, rows, row_step, band_row0;
};
PartRows part_rows(int32_t height, int32_t k, int32_t parts, int32_t j, int32_t p);

}  // namespace vrt

#pragma GCC visibility pop

#endif  // VRT_BANDS_H
