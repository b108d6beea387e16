// The scene-cut signature of a frame (modules/scene_cuts.py restates it on the host, bit for bit): a 4 x 4 grid of 16-bin luma
// histograms of a uint8 BGR frame, in integer arithmetic throughout:
//     Y = (29 * B + 150 * G + 77 * R + 128) >> 8,  bin = Y >> 4,  cell = ((y * 4) / H) * 4 + (x * 4) / W,  sig[n][cell * 16 + bin] += 1.
// Declared in include/keep_cv_hip.h.
//
// One block = a band of rows of ONE cell of one frame, so every pixel a lane meets goes to the same 16 counters and the lane keeps them
// to itself: 16 counters of 8 bits in two 64-bit registers.  Real video puts most pixels of a cell into one to three bins -- a flat frame
// into one -- so a histogram that is shared from the first add (LDS atomics per pixel) serialises on exactly the frames that matter; a
// lane's own counters never collide.  A lane takes at most SG_ITER groups of 4 pixels (64 adds: no 8-bit counter overflows), the wave sums
// its lanes' counters as 16-bit pairs by shuffles (64 lanes x 64 = 4096 < 65536), the four waves meet in LDS, and the block adds its 16
// totals to the frame's counters with vector global atomics on integers: the sums do not depend on the order of arrival, on N, or on
// the launch geometry.  The counters are zeroed by a kernel of their own on the same stream in front.
//
// Loads: a group of 4 pixels is 12 bytes at a pixel boundary, inside the cell's row segment by construction (no byte outside the frame
// is read).  `frames` needs no alignment -- the store hands out views, and a row of an odd width starts anywhere -- so the 12 bytes are
// read as they lie (gfx950 under HSA serves unaligned global loads); the 1 - 3 pixels at the end of a row segment are read byte by byte.
#include <string.h>

#include "keep_common.h"
#include "../../include/keep_cv_hip.h"

#define SG_THREADS 256
#define SG_ITER 16                      // groups of 4 pixels per lane at most: 64 adds per 8-bit counter

struct SigP {
  const uint8_t* frames;
  int32_t* sig;
  int H, W;
  int rpb, parts;                       // rows per block; blocks per cell
};

// first row (column) of cell row (column) c: the smallest y with (y * 4) / H >= c
__host__ __device__ static inline int sg_first(int c, int S) { return (c * S + 3) >> 2; }

__device__ __forceinline__ void sg_count(uint32_t b, uint32_t g, uint32_t r, uint64_t& lo, uint64_t& hi) {
  const uint32_t bin = (29u * b + 150u * g + 77u * r + 128u) >> 12;       // (Y >> 4, Y <= 255: bin <= 15)
  const uint64_t inc = 1ull << ((bin & 7u) * 8u);
  lo += (bin & 8u) ? 0ull : inc;
  hi += (bin & 8u) ? inc : 0ull;
}

__global__ void __launch_bounds__(64) signature_zero_kernel(int32_t* sig, long n) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i < n) sig[i] = 0;
}

__global__ void __launch_bounds__(SG_THREADS) frame_signature_u8_kernel(SigP p) {
  __shared__ uint32_t part[SG_THREADS / 64][16];
  const int tid = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  const int band = (int)(blk % (uint32_t)p.parts);
  const int cell = (int)((blk / (uint32_t)p.parts) & 15u);
  const long n = blk / ((uint32_t)p.parts * 16u);
  const int cy = cell >> 2, cx = cell & 3;
  const int x0 = sg_first(cx, p.W), x1 = sg_first(cx + 1, p.W);
  const int ya = sg_first(cy, p.H) + band * p.rpb;
  const int yb = min(ya + p.rpb, sg_first(cy + 1, p.H));
  const int cw = x1 - x0;
  if (cw <= 0 || yb <= ya) return;      // an empty cell (H or W below 4), or a band past the cell's last row: uniform over the block
  const int gpr = (cw + 3) >> 2;        // groups per row, the last one of 1 - 4 pixels
  const int total = (yb - ya) * gpr;    // <= SG_THREADS * SG_ITER by the launcher's rpb
  const uint8_t* frame = p.frames + n * ((long)p.H * p.W * 3);

  uint64_t lo = 0, hi = 0;
#pragma unroll 4
  for (int i = tid; i < total; i += SG_THREADS) {
    const int row = i / gpr, g = i - row * gpr;
    const int x = x0 + 4 * g;
    const uint8_t* s = frame + ((long)(ya + row) * p.W + x) * 3;
    if (x + 4 <= x1) {
      uint32_t w[3];
      memcpy(w, s, 12);
      sg_count(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u, lo, hi);
      sg_count(w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u, lo, hi);
      sg_count((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u, lo, hi);
      sg_count((w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24, lo, hi);
    } else {
      for (int k = 0; k < x1 - x; ++k) sg_count(s[3 * k], s[3 * k + 1], s[3 * k + 2], lo, hi);
    }
  }

  // the lane's 16 counters as 8 pairs of 16 bits, summed over the wave
  uint32_t r[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    r[j] = (uint32_t)((lo >> (16 * j)) & 255u) | ((uint32_t)((lo >> (16 * j + 8)) & 255u) << 16);
    r[4 + j] = (uint32_t)((hi >> (16 * j)) & 255u) | ((uint32_t)((hi >> (16 * j + 8)) & 255u) << 16);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += (uint32_t)__shfl_xor((int)r[j], d, 64);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      part[tid >> 6][2 * j] = r[j] & 0xffffu;
      part[tid >> 6][2 * j + 1] = r[j] >> 16;
    }
  }
  __syncthreads();
  if (tid < 16) {
    uint32_t v = 0;
#pragma unroll
    for (int w = 0; w < SG_THREADS / 64; ++w) v += part[w][tid];
    if (v) atomicAdd(p.sig + n * 256 + cell * 16 + tid, (int32_t)v);
  }
}

extern "C" int32_t keep_frame_signature_u8(const uint8_t* frames, int32_t N, int32_t H, int32_t W, int32_t* sig, void* stream) {
  KEEP_REQUIRE(frames && sig, "keep_frame_signature_u8: null pointer");
  KEEP_REQUIRE(N > 0 && H > 0 && W > 0, "keep_frame_signature_u8: sizes must be positive (N=%d H=%d W=%d)", N, H, W);
  KEEP_REQUIRE(H < 32768 && W < 32768, "keep_frame_signature_u8: H and W must be below 32768 (H=%d W=%d)", H, W);
  // the widest cell column has at most ceil(W / 4) pixels; a block takes as many rows of it as SG_THREADS * SG_ITER groups hold
  const int gpr_max = ((W + 3) / 4 + 3) / 4;                      // <= 2048: a row always fits
  const int rpb = (SG_THREADS * SG_ITER) / gpr_max;
  const int parts = cdiv((H + 3) / 4, rpb);                       // the tallest cell row has at most ceil(H / 4) rows
  const long per_frame = 16L * parts;
  const long cap = (1L << 30) / per_frame;                        // frames per launch: the grid's x extent stays below 2^31
  hipStream_t st = (hipStream_t)stream;
  const long cells = (long)N * 256;
  for (long z = 0; z < cells; z += 64L << 20) {
    const long m = cells - z < (64L << 20) ? cells - z : (64L << 20);
    hipLaunchKernelGGL(signature_zero_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, st, sig + z, m);
  }
  KEEP_LAUNCH_CHECK("keep_frame_signature_u8");
  for (long n0 = 0; n0 < N; n0 += cap) {
    const long m = N - n0 < cap ? N - n0 : cap;
    SigP p;
    p.frames = frames + n0 * ((long)H * W * 3);
    p.sig = sig + n0 * 256;
    p.H = H; p.W = W; p.rpb = rpb; p.parts = parts;
    hipLaunchKernelGGL(frame_signature_u8_kernel, dim3((unsigned)(m * per_frame)), dim3(SG_THREADS), 0, st, p);
  }
  KEEP_LAUNCH_CHECK("keep_frame_signature_u8");
  return KEEP_OK;
}
