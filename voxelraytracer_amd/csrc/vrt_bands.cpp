// vrt_bands.cpp — the band plans: which frame rows each of k devices, parts or ranks renders, the 2-D copies
// that place a band into its frame rows, and the vrt_*_plan entry points that publish them (vrt_bands.h).
// Integer arithmetic only: it calls nothing of the HIP or RCCL runtime and includes neither's headers, so a
// plain host compiler builds and links it without either library.
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "vrt.h"
#include "vrt_bands.h"

namespace vrt {

// Cyclic-row bands (ABI v8/v10 plans): band j holds frame rows j, j + k, ...
static int32_t cyc_band_rows(int32_t height, int32_t k, int32_t j) { return j < height ? (height - j + k - 1) / k : 0; }

BandGeom block_band(int32_t height, int32_t k, int32_t block, int32_t j) {
  if (k == 1) return BandGeom{0, height, 1, 0};
  int32_t sh = 0;
  while ((1 << sh) < block) ++sh;
  const int32_t nb = (height + block - 1) / block;
  const int32_t own = j < nb ? (nb - j + k - 1) / k : 0;
  int32_t rows = own * block;
  if (own > 0 && (nb - 1) % k == j) rows -= nb * block - height;
  return BandGeom{j * block, rows, k * block, sh};
}
// rows of the largest of the k bands (band 0 unless it also owns the short last block)
int32_t largest_band(int32_t height, int32_t k, int32_t block) {
  int32_t m = 0;
  for (int32_t j = 0; j < k; ++j) m = std::max(m, block_band(height, k, block, j).rows);
  return m;
}
int32_t frame_block(int32_t k) { return k > 1 ? kFrameRowBlock : 1; }
int32_t band_rows(int32_t height, int32_t k, int32_t j) { return block_band(height, k, frame_block(k), j).rows; }
// rows of the largest band (band 0's): every band buffer and the gather's per-device slice
int32_t band_cap(int32_t height, int32_t k) {
  if (k == 1) return height;
  const int32_t nb = (height + kFrameRowBlock - 1) / kFrameRowBlock;
  return (nb + k - 1) / k * kFrameRowBlock;
}

// The 2-D copies that place band j (its rows packed at `row` bytes each) into its frame rows:
// cyclic rows (block 1) are one copy of `rows` rows k rows apart; block-cyclic bands one copy of
// the band's full blocks (block x row bytes each, k blocks apart) and one of a short last block.
// Staging to the host and the device-to-device assembly use exactly these (vrt_block_copy_plan).
int band_copies(int32_t w, int32_t h, int32_t k, int32_t block, int32_t j, size_t elem, BandCopy out[2]) {
  const size_t row = size_t(w) * elem;
  if (block == 1) {
    out[0] = BandCopy{size_t(j) * row, size_t(k) * row, 0, row, row, size_t(cyc_band_rows(h, k, j))};
    return out[0].rows ? 1 : 0;
  }
  const BandGeom g = block_band(h, k, block, j);
  const size_t full = size_t(g.rows) / size_t(block), rest = size_t(g.rows) % size_t(block);
  int n = 0;
  if (full) out[n++] = BandCopy{size_t(j) * block * row, size_t(k) * block * row, 0, size_t(block) * row,
                                size_t(block) * row, full};
  if (rest) out[n++] = BandCopy{(full * size_t(k) + size_t(j)) * size_t(block) * row, rest * row,
                                full * size_t(block) * row, rest * row, rest * row, 1};
  return n;
}

PartRows part_rows(int32_t height, int32_t k, int32_t parts, int32_t j, int32_t p) {
  const int32_t hb = cyc_band_rows(height, k, j);
  return PartRows{j + p * k, hb > p ? (hb - p + parts - 1) / parts : 0, k * parts, p};
}

}  // namespace vrt

using namespace vrt;

extern "C" {

int vrt_band_plan(int32_t height, int32_t k, int32_t parts, int32_t* out) {
  if (height < 1 || k < 1 || parts < 1 || !out) return VRT_ERR_INVALID;
  for (int32_t j = 0; j < k; ++j)
    for (int32_t p = 0; p < parts; ++p) {
      const PartRows pr = part_rows(height, k, parts, j, p);
      int32_t* o = out + (size_t(j) * parts + p) * 4;
      o[0] = pr.row0;
      o[1] = pr.rows;
      o[2] = pr.row_step;
      o[3] = pr.band_row0;
    }
  return (height + k - 1) / k;  // the largest cyclic band
}

int vrt_band_copy_plan(int32_t width, int32_t height, int32_t k, int32_t elem_bytes, int64_t* out) {
  if (width < 1 || height < 1 || k < 1 || elem_bytes < 1 || !out) return VRT_ERR_INVALID;
  for (int32_t j = 0; j < k; ++j) {
    BandCopy bc[2];
    const int nc = band_copies(width, height, k, 1, j, size_t(elem_bytes), bc);
    int64_t* o = out + size_t(j) * 5;
    o[0] = int64_t(bc[0].dst_off);
    o[1] = int64_t(bc[0].dst_pitch);
    o[2] = int64_t(bc[0].src_pitch);
    o[3] = int64_t(bc[0].width);
    o[4] = nc ? int64_t(bc[0].rows) : 0;
  }
  return k;
}

int vrt_frame_row_block(int32_t k) { return k < 1 ? VRT_ERR_INVALID : frame_block(k); }

int vrt_block_band_plan(int32_t height, int32_t k, int32_t row_block, int32_t* out) {
  if (height < 1 || k < 1 || !out || row_block < 1 || row_block > 64 || (row_block & (row_block - 1)))
    return VRT_ERR_INVALID;
  int32_t cap = 0;
  for (int32_t j = 0; j < k; ++j) {
    // k = 1: the whole frame as one band of blocks row_block apart (the same row formula)
    const BandGeom g = k == 1 ? BandGeom{0, height, row_block, 0} : block_band(height, k, row_block, j);
    out[size_t(j) * 3 + 0] = g.row0;
    out[size_t(j) * 3 + 1] = g.rows;
    out[size_t(j) * 3 + 2] = g.row_step;
    cap = std::max(cap, g.rows);
  }
  return cap;
}

int vrt_block_copy_plan(int32_t width, int32_t height, int32_t k, int32_t row_block, int32_t elem_bytes,
                        int64_t* out) {
  if (width < 1 || height < 1 || k < 1 || elem_bytes < 1 || !out || row_block < 1 || row_block > 64 ||
      (row_block & (row_block - 1)))
    return VRT_ERR_INVALID;
  int n = 0;
  for (int32_t j = 0; j < k; ++j) {
    BandCopy bc[2];
    const int nc = k == 1 ? band_copies(width, height, 1, 1, 0, size_t(elem_bytes), bc)
                          : band_copies(width, height, k, row_block, j, size_t(elem_bytes), bc);
    for (int c = 0; c < 2; ++c) {
      int64_t* o = out + (size_t(j) * 2 + c) * 7;
      const BandCopy b = c < nc ? bc[c] : BandCopy{0, 0, 0, 0, 0, 0};
      o[0] = j;
      o[1] = int64_t(b.dst_off);
      o[2] = int64_t(b.dst_pitch);
      o[3] = int64_t(b.src_off);
      o[4] = int64_t(b.src_pitch);
      o[5] = int64_t(b.width);
      o[6] = int64_t(b.rows);
      n += c < nc ? 1 : 0;
    }
  }
  return n;
}

}  // extern "C"
