/* skipfield_fast.c: a fast exact restatement of the packed skip field, for the tests alone
 * (tests/skipfield_reference.py builds and loads it). Independent of the kernels' separable
 * min / max scans and of the prefix-sum brute force of skipfield_reference.py:
 *
 *   F of an octant (step s): the largest-empty-cube dynamic programme, swept against s.
 *     F(v) = 0 for a non-empty voxel, else 1 + min of F over the seven neighbours
 *     v + s * ({0,1}^3 \ {0}); F outside the volume is 0; clamped to cap.
 *     (A cube of edge E anchored at v is empty exactly when v is empty and the seven cubes of
 *     edge E - 1 anchored at those neighbours are; min(cap, 1 + min(min(cap, F_i))) equals
 *     min(cap, 1 + min F_i), so clamping inside the sweep is exact.)
 *     G(w) = max(F(w - s) - 1, 0), 0 where w - s is outside.
 *   D: the two-pass 26-neighbour chamfer, exact for the chessboard metric; the outside counts as
 *     non-empty; clamped to cap.
 *
 * Volumes are n^3 bytes, x fastest ([z][y][x]). Work arrays are padded by one cell of zeros on every
 * side, which is the outside. cap <= 255. Every function returns 0, or -1 for a bad argument or a
 * failed allocation. */
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int bad(const void* a, const void* b, int n, int cap) {
  return !a || !b || n < 1 || n > 1024 || cap < 1 || cap > 255;
}

/* f: (n+2)^3 bytes, zeroed by the caller; filled with F of `octant` at [k+1][j+1][i+1] */
static void forward_padded(const uint8_t* vox, int n, int octant, int cap, uint8_t* f) {
  const int sx = octant & 1 ? -1 : 1, sy = octant & 2 ? -1 : 1, sz = octant & 4 ? -1 : 1;
  const size_t p = (size_t)n + 2;
  const ptrdiff_t dx = sx, dy = sy * (ptrdiff_t)p, dz = sz * (ptrdiff_t)(p * p);
  for (int kk = 0; kk < n; ++kk) {
    const int k = sz > 0 ? n - 1 - kk : kk;
    for (int jj = 0; jj < n; ++jj) {
      const int j = sy > 0 ? n - 1 - jj : jj;
      const uint8_t* row = vox + ((size_t)k * n + j) * n;
      uint8_t* fr = f + ((size_t)(k + 1) * p + (size_t)(j + 1)) * p + 1;
      for (int ii = 0; ii < n; ++ii) {
        const int i = sx > 0 ? n - 1 - ii : ii;
        if (row[i]) {
          fr[i] = 0;
          continue;
        }
        const uint8_t* q = fr + i;
        int m = q[dx];
        if (q[dy] < m) m = q[dy];
        if (q[dx + dy] < m) m = q[dx + dy];
        if (q[dz] < m) m = q[dz];
        if (q[dz + dx] < m) m = q[dz + dx];
        if (q[dz + dy] < m) m = q[dz + dy];
        if (q[dz + dx + dy] < m) m = q[dz + dx + dy];
        fr[i] = (uint8_t)(m + 1 < cap ? m + 1 : cap);
      }
    }
  }
}

/* d: (n+2)^3 bytes, zeroed by the caller; filled with D at [k+1][j+1][i+1] */
static void chamfer_padded(const uint8_t* vox, int n, int cap, uint8_t* d) {
  const size_t p = (size_t)n + 2;
  const ptrdiff_t sy = (ptrdiff_t)p, sz = (ptrdiff_t)(p * p);
  ptrdiff_t nb[13]; /* the 13 neighbours that come earlier in raster order */
  int c = 0;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b) nb[c++] = -sz + a * sy + b;
  for (int b = -1; b <= 1; ++b) nb[c++] = -sy + b;
  nb[c++] = -1;
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j) {
      const uint8_t* row = vox + ((size_t)k * n + j) * n;
      uint8_t* dr = d + ((size_t)(k + 1) * p + (size_t)(j + 1)) * p + 1;
      for (int i = 0; i < n; ++i) {
        if (row[i]) {
          dr[i] = 0;
          continue;
        }
        int m = cap - 1;
        for (int t = 0; t < 13; ++t)
          if (dr[i + nb[t]] < m) m = dr[i + nb[t]];
        dr[i] = (uint8_t)(m + 1);
      }
    }
  for (int k = n - 1; k >= 0; --k)
    for (int j = n - 1; j >= 0; --j) {
      uint8_t* dr = d + ((size_t)(k + 1) * p + (size_t)(j + 1)) * p + 1;
      for (int i = n - 1; i >= 0; --i) {
        int m = dr[i];
        if (m == 0) continue;
        for (int t = 0; t < 13; ++t)
          if (dr[i - nb[t]] + 1 < m) m = dr[i - nb[t]] + 1;
        dr[i] = (uint8_t)m;
      }
    }
}

static void unpad(const uint8_t* f, int n, uint8_t* out) {
  const size_t p = (size_t)n + 2;
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      memcpy(out + ((size_t)k * n + j) * n, f + ((size_t)(k + 1) * p + (size_t)(j + 1)) * p + 1, (size_t)n);
}

/* out: n^3 bytes, F of `octant` (bit a set: the step is -1 on axis a; x is axis 0) at every anchor */
int sf_forward(const uint8_t* vox, int n, int octant, int cap, uint8_t* out) {
  if (bad(vox, out, n, cap) || octant < 0 || octant > 7) return -1;
  const size_t p = (size_t)n + 2;
  uint8_t* f = calloc(p * p * p, 1);
  if (!f) return -1;
  forward_padded(vox, n, octant, cap, f);
  unpad(f, n, out);
  free(f);
  return 0;
}

/* out: n^3 bytes, D at every voxel */
int sf_chebyshev(const uint8_t* vox, int n, int cap, uint8_t* out) {
  if (bad(vox, out, n, cap)) return -1;
  const size_t p = (size_t)n + 2;
  uint8_t* d = calloc(p * p * p, 1);
  if (!d) return -1;
  chamfer_padded(vox, n, cap, d);
  unpad(d, n, out);
  free(d);
  return 0;
}

/* One packed (n+1)^3 volume: voxel | skip << 8 in [0, n)^3, where skip is G from the padded F of
 * step (sx, sy, sz), or, with s = 0 on every axis, the padded D itself; texel n of an axis repeats
 * voxel 0 of that axis with skip distance 0. */
static void pack(const uint8_t* vox, const uint8_t* f, int n, int sx, int sy, int sz, uint16_t* out) {
  const size_t p = (size_t)n + 2, q = (size_t)n + 1;
  const int centred = sx == 0;
  for (int k = 0; k <= n; ++k)
    for (int j = 0; j <= n; ++j) {
      const uint8_t* row = vox + ((size_t)(k % n) * n + (size_t)(j % n)) * n;
      uint16_t* o = out + ((size_t)k * q + j) * q;
      if (k == n || j == n) {
        for (int i = 0; i <= n; ++i) o[i] = row[i % n];
        continue;
      }
      const uint8_t* fr = f + ((size_t)(k + 1 - sz) * p + (size_t)(j + 1 - sy)) * p + 1 - sx;
      for (int i = 0; i < n; ++i) {
        const int v = fr[i];
        const int g = centred ? v : (v > 0 ? v - 1 : 0);
        o[i] = (uint16_t)(row[i] | g << 8);
      }
      o[n] = row[0];
    }
}

/* out: [octants][n+1]^3 u16, the whole layout of the device's packed volume(s). octants 8: the
 * forward distances with cap fwd_cap, octant by octant (in parallel, at most 16 threads);
 * octants 1: the centred distance with cap dist_cap. */
int sf_packed(const uint8_t* vox, int n, int octants, int fwd_cap, int dist_cap, uint16_t* out) {
  if (bad(vox, out, n, octants == 8 ? fwd_cap : dist_cap) || (octants != 8 && octants != 1)) return -1;
  const size_t p = (size_t)n + 2, q = (size_t)n + 1;
  int fail = 0;
  if (octants == 1) {
    uint8_t* d = calloc(p * p * p, 1);
    if (!d) return -1;
    chamfer_padded(vox, n, dist_cap, d);
    pack(vox, d, n, 0, 0, 0, out);
    free(d);
    return 0;
  }
#pragma omp parallel for num_threads(8) schedule(dynamic, 1)
  for (int o = 0; o < 8; ++o) {
    uint8_t* f = calloc(p * p * p, 1);
    if (!f) {
#pragma omp atomic write
      fail = 1;
      continue;
    }
    forward_padded(vox, n, o, fwd_cap, f);
    pack(vox, f, n, o & 1 ? -1 : 1, o & 2 ? -1 : 1, o & 4 ? -1 : 1, out + (size_t)o * q * q * q);
    free(f);
  }
  return fail ? -1 : 0;
}
