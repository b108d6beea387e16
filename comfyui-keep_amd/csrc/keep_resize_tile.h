// Tile I/O and launch plumbing shared by the three OpenCV-exact uint8 resizes (keep_resize.hip, keep_resize_area.hip,
// keep_resize_linear.hip).  Each of them works on an output tile of one frame of a contiguous [N,H,W,3] -> [N,H2,W2,3] launch: it stages
// the tile's source rectangle in LDS as the 16-byte words that hold it, builds the uint8 tile in LDS at the byte phase of its
// destination, and writes it in 16-byte stores.  Neither the frames nor their rows need any alignment.  The pixel arithmetic and the
// tables are the kernels' own.
#pragma once
#include "keep_common.h"

#define RT_THREADS 256                 // block size of the three kernels; the loops below stride by it
#define RT_TW 64                       // output pixels per tile row (at most)
#define RT_OROW (RT_TW * 3 + 16)       // uint8 output tile row in LDS: 192 bytes + the destination's 16-byte phase

// Byte phase, within its 16-byte word, of pixel (row, col) of the frame at `base`, whose rows are W pixels wide: where a staged row's
// first byte sits in its LDS row (rt_stage), and where a tile row starts in its row of the output tile (rt_store_tile).
// (only the low 4 bits of an address matter for a 16-byte phase: 32-bit arithmetic)
__device__ __forceinline__ int rt_phase(const uint8_t* base, int row, int W, int col) {
  return (int)(((uint32_t)reinterpret_cast<uintptr_t>(base) + ((uint32_t)row * (uint32_t)W + (uint32_t)col) * 3u) & 15u);
}

// Stages rows [0, R) of a source rectangle: sb[r * srow ...] receives the 16-byte words that hold bytes [(row_of(r) * W + cx_lo) * 3,
// ... + ncol_b) of the frame at `src`, so the first of them lands at sb[r * srow + rt_phase(src, row_of(r), W, cx_lo)].  row_of is a
// callable (a lambda inlines): the Lanczos kernel clamps its rows into the frame one by one, the other two stage consecutive rows.
// srow is a multiple of 16 and at least ncol_b + 15.  The caller synchronises.
template <class RowOf>
__device__ __forceinline__ void rt_stage(uint8_t* sb, int srow, const uint8_t* src, int W, int cx_lo, int ncol_b, int R, RowOf row_of) {
  const int nchunk = srow >> 4;
  for (int i = threadIdx.x; i < R * nchunk; i += RT_THREADS) {
    const int r = i / nchunk, k = i - r * nchunk;
    const uint8_t* b0 = src + ((long)row_of(r) * W + cx_lo) * 3;
    const uint8_t* a0 = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(b0) & ~(uintptr_t)15);
    // (a word that holds at least one byte of the row segment lies in a page of the buffer: reading all of it cannot fault)
    if (16 * k < (int)(b0 - a0) + ncol_b)
      *reinterpret_cast<uint4*>(sb + (long)r * srow + 16 * k) = *reinterpret_cast<const uint4*>(a0 + 16 * k);
  }
}

// Writes tile rows [0, th) of hw bytes each, built at ot[y * RT_OROW + rt_phase(dst, y0 + y, W2, x0) ...], to dst + ((y0 + y) * W2 + x0) * 3:
// per tile row, the 16-byte words that lie wholly inside its destination segment, then the bytes at its two ends.  The caller has
// synchronised after building ot.
__device__ __forceinline__ void rt_store_tile(const uint8_t* ot, uint8_t* dst, int W2, int x0, int y0, int th, int hw) {
  const int nw = RT_OROW >> 4;
  for (int i = threadIdx.x; i < th * nw; i += RT_THREADS) {
    const int y = i / nw, k = i - y * nw;
    uint8_t* d0 = dst + ((long)(y0 + y) * W2 + x0) * 3;
    const int phase = (int)(reinterpret_cast<uintptr_t>(d0) & 15);
    const int lo = 16 * k - phase, hi = lo + 16;                   // the word's bytes relative to the segment start
    if (lo >= 0 && hi <= hw)
      *reinterpret_cast<uint4*>(d0 + lo) = *reinterpret_cast<const uint4*>(&ot[y * RT_OROW + 16 * k]);
  }
  for (int i = threadIdx.x; i < th * 32; i += RT_THREADS) {
    const int y = i >> 5, j = i & 31;
    uint8_t* d0 = dst + ((long)(y0 + y) * W2 + x0) * 3;
    const int phase = (int)(reinterpret_cast<uintptr_t>(d0) & 15);
    const int head = min((16 - phase) & 15, hw);                   // bytes before the first whole word
    const int body_end = head + ((hw - head) & ~15);
    const int e = j < 16 ? j : body_end + (j - 16);                // j < 16: head byte j; else tail byte j - 16
    if ((j < 16 && e < head) || (j >= 16 && e < hw)) d0[e] = ot[y * RT_OROW + phase + e];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// The argument checks every [N,H,W,3] -> [N,H2,W2,3] launch makes; `name` (the entry) opens the messages, `ptrs`: no pointer is null.
static inline int32_t rt_check_args(const char* name, bool ptrs, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2) {
  KEEP_REQUIRE(ptrs, "%s: null pointer", name);
  KEEP_REQUIRE(N > 0 && H > 0 && W > 0 && H2 > 0 && W2 > 0, "%s: sizes must be positive (N=%d H=%d W=%d H2=%d W2=%d)", name, N, H, W, H2, W2);
  KEEP_REQUIRE(W <= INT32_MAX / 3 && W2 <= INT32_MAX / 3, "%s: W * 3 or W2 * 3 overflows int32 (W=%d W2=%d)", name, W, W2);
  KEEP_REQUIRE(N <= 65535, "%s: at most 65535 frames per call, got %d", name, N);
  return KEEP_OK;
}

// The grid of tiles of th rows x tw pixels over N frames of checked sizes.
static inline int32_t rt_grid(const char* name, int32_t N, int32_t H2, int32_t W2, int th, int tw, dim3& grid) {
  grid = dim3(cdiv(W2, tw), cdiv(H2, th), N);
  KEEP_REQUIRE(grid.y <= 65535, "%s: output too tall (H2=%d)", name, H2);
  return KEEP_OK;
}

// Halves th or tw (powers of two; th while it is at least half of tw) until bytes(th, tw), the dynamic LDS of such a tile, fits lds_cap
// or the tile is one pixel.  The last call of `bytes` is for the shape that is left, so the capacities it computed on the way are that
// shape's.
template <class Bytes>
static inline void rt_fit_tile(int& th, int& tw, long lds_cap, Bytes bytes) {
  while (bytes(th, tw) > lds_cap && !(th == 1 && tw == 1)) {
    if (th > 1 && (th >= tw / 2 || tw == 1)) th >>= 1;
    else tw >>= 1;
  }
}

// log2 of a tile width (a power of two); the 4-byte row stride of a tile's horizontal sums: tw * 3 rounded up to 4
static inline int rt_lg(int tw) {
  int lg = 0;
  while ((1 << lg) < tw) ++lg;
  return lg;
}
static inline int rt_hs(int tw) { return (tw * 3 + 3) & ~3; }
