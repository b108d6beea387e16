// cv2.resize(src uint8 [H,W,3], (W2, H2), interpolation=INTER_LANCZOS4) on the device: the background resize of
// final_upscale_factor (face_restoration_helper.py:354-356, keep_processor.py:139-142,283-286 of the reference).
// OpenCV 4.x modules/imgproc/src/resize.cpp (resizeGeneric_, HResizeLanczos4<uchar,int,short,2048>, VResizeLanczos4 with
// FixedPtCast<int,uchar,22>, interpolateLanczos4): per axis a table of 8 int16 coefficients (scale 2048) and one source
// offset per destination index; tap i of destination d reads source clamp(ofs[d] - 3 + i, 0, S - 1).  Both passes are exact
// int32 sums, so their order does not matter: the tables are the only delicate part, and they are built on the host
// (keep_lanczos4_tables) with OpenCV's own double / float operation sequence, FMA contraction off (Makefile).
#include <math.h>

#include "keep_common.h"

#pragma clang fp contract(off)

// ---- tables (host C: no device needed) ----------------------------------------------------------------------------------
static void lanczos4_coeffs(float x, float* coeffs) {
  static const double s45 = 0.70710678118654752440084436210485;
  static const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
  const double pi = 3.1415926535897932384626433832795;
  float sum = 0.f;
  const double y0 = -(double)(x + 3.0f) * pi * 0.25, s0 = std::sin(y0), c0 = std::cos(y0);
  for (int i = 0; i < 8; ++i) {
    const float y0_ = (x + 3.0f) - (float)i;
    if (fabsf(y0_) >= 1e-6f) {
      const double y = -(double)y0_ * pi * 0.25;
      coeffs[i] = (float)((cs[i][0] * s0 + cs[i][1] * c0) / (y * y));
    } else {
      coeffs[i] = 1e30f;             // x == 0: the centre tap dominates the sum and normalises to 1
    }
    sum += coeffs[i];
  }
  const float inv = 1.0f / sum;
  for (int i = 0; i < 8; ++i) coeffs[i] *= inv;
}

extern "C" int32_t keep_lanczos4_tables(int32_t S, int32_t D, int32_t* ofs, int16_t* coef) {
  KEEP_REQUIRE(ofs && coef && S > 0 && D > 0, "keep_lanczos4_tables: bad arguments (S=%d, D=%d)", S, D);
  const double scale = 1.0 / ((double)D / S);
  for (int d = 0; d < D; ++d) {
    float f = (float)((d + 0.5) * scale - 0.5);
    const int s = (int)floorf(f);
    f -= (float)s;
    ofs[d] = s;
    float c[8];
    lanczos4_coeffs(f, c);
    for (int i = 0; i < 8; ++i) {
      const int v = (int)lrintf(c[i] * 2048.0f);          // cvRound: round half to even
      coef[d * 8 + i] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
    }
  }
  return KEEP_OK;
}

// ---- kernel ---------------------------------------------------------------------------------------------------------------
// One block = an output tile of th rows x tw pixels of one frame (blockIdx.z).  Its source footprint -- rows
// [yofs[y0] - 3, yofs[y1 - 1] + 4] (clamped row by row), columns [xofs[x0] - 3, xofs[x1 - 1] + 4] -- is staged in LDS with
// 16-byte loads, the horizontal pass writes int32 [rows][tw * 3] to LDS, the vertical pass writes the uint8 tile to LDS at the
// byte phase of its destination, and each tile row leaves in 16-byte stores (single bytes only where the row segment starts or
// ends inside a 16-byte word).  The host sizes th / tw so that the footprint fits the dynamic LDS it passes (rcap rows of srow
// bytes); the kernel clamps to those capacities all the same.
#define RZ_TW 64                       // output pixels per tile row (at most)
#define RZ_TH 32                       // output rows per tile (at most)
#define RZ_OROW (RZ_TW * 3 + 16)       // uint8 output tile row in LDS: 192 bytes + the destination's 16-byte phase

struct ResizeP {
  const uint8_t* src;
  uint8_t* dst;
  const int32_t* xofs;
  const int16_t* xcoef;
  const int32_t* yofs;
  const int16_t* ycoef;
  int H, W, H2, W2;
  int tw, th, rcap, srow;              // tile shape, staged source rows / bytes per staged row (dynamic LDS)
  int lg_tw, hs;                       // log2(tw); int32 row stride of the horizontal sums (tw * 3 rounded up to 4)
};

__global__ void __launch_bounds__(256) resize_lanczos4_u8_kernel(ResizeP p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rz_dyn[];
  __shared__ int xo[RZ_TW], yo[RZ_TH];
  __shared__ __attribute__((aligned(16))) int16_t xc[RZ_TW * 8], yc[RZ_TH * 8];
  __shared__ __attribute__((aligned(16))) uint8_t ot[RZ_TH * RZ_OROW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * p.tw, y0 = blockIdx.y * p.th;
  const int tw = min(p.tw, p.W2 - x0), th = min(p.th, p.H2 - y0);
  const long n = blockIdx.z;
  const uint8_t* src = p.src + n * p.H * (long)p.W * 3;
  uint8_t* dst = p.dst + n * p.H2 * (long)p.W2 * 3;

  for (int i = tid; i < tw; i += 256) {
    xo[i] = p.xofs[x0 + i];
    *reinterpret_cast<int4*>(&xc[i * 8]) = *reinterpret_cast<const int4*>(&p.xcoef[(long)(x0 + i) * 8]);
  }
  for (int i = tid; i < th; i += 256) {
    yo[i] = p.yofs[y0 + i];
    *reinterpret_cast<int4*>(&yc[i * 8]) = *reinterpret_cast<const int4*>(&p.ycoef[(long)(y0 + i) * 8]);
  }
  __syncthreads();

  // source footprint of the tile
  const int sy0 = yo[0] - 3;
  const int R = min(yo[th - 1] + 4 - sy0 + 1, p.rcap);
  const int cx_lo = max(xo[0] - 3, 0), cx_hi = min(xo[tw - 1] + 4, p.W - 1);
  const int ncol_b = (cx_hi - cx_lo + 1) * 3;
  uint8_t* sb = rz_dyn;                                              // [rcap][srow] staged source bytes
  int* hb = reinterpret_cast<int*>(rz_dyn + (long)p.rcap * p.srow);  // [rcap][hs] horizontal sums
  const int hw = tw * 3, hs = p.hs;
  // (only the low 4 bits of an address matter for a 16-byte phase: 32-bit arithmetic)
  const uint32_t src_lo = (uint32_t)reinterpret_cast<uintptr_t>(src), dst_lo = (uint32_t)reinterpret_cast<uintptr_t>(dst);

  // stage: row r of the footprint is source row clamp(sy0 + r); its columns [cx_lo, cx_hi] as the 16-byte words that hold them
  const int nchunk = p.srow >> 4;
  for (int i = tid; i < R * nchunk; i += 256) {
    const int r = i / nchunk, k = i - r * nchunk;
    const int row = min(max(sy0 + r, 0), p.H - 1);
    const uint8_t* b0 = src + ((long)row * p.W + cx_lo) * 3;
    const uint8_t* a0 = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(b0) & ~(uintptr_t)15);
    // (a word that holds at least one byte of the row segment lies in a page of the buffer: reading all of it cannot fault)
    if (16 * k < (int)(b0 - a0) + ncol_b)
      *reinterpret_cast<uint4*>(sb + (long)r * p.srow + 16 * k) = *reinterpret_cast<const uint4*>(a0 + 16 * k);
  }
  __syncthreads();

  // horizontal pass: hb[r][x * 3 + c] = sum_i src[row][clamp(xofs[x] - 3 + i)][c] * xcoef[x][i]
  for (int i = tid; i < (R << p.lg_tw); i += 256) {
    const int r = i >> p.lg_tw, x = i & (p.tw - 1);
    if (x >= tw) continue;
    const int row = min(max(sy0 + r, 0), p.H - 1);
    const int phase = (int)((src_lo + ((uint32_t)row * (uint32_t)p.W + (uint32_t)cx_lo) * 3u) & 15u);
    const uint8_t* s = sb + (long)r * p.srow + phase;
    const int4 cw = *reinterpret_cast<const int4*>(&xc[x * 8]);
    const int16_t* a = reinterpret_cast<const int16_t*>(&cw);
    const int base = xo[x] - 3;
    int h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int col = (min(max(base + t, 0), p.W - 1) - cx_lo) * 3;
      const int w = a[t];
      h0 += (int)s[col] * w;
      h1 += (int)s[col + 1] * w;
      h2 += (int)s[col + 2] * w;
    }
    int* h = hb + r * hs + x * 3;
    h[0] = h0; h[1] = h1; h[2] = h2;
  }
  __syncthreads();

  // vertical pass: dst[y][x][c] = clamp((sum_k hb[yofs[y] - 3 + k - sy0][x][c] * ycoef[y][k] + 2^21) >> 22, 0, 255); a lane owns 4
  // consecutive bytes of a tile row (16-byte LDS reads), a wave a row
  const int ve = 4 * (tid & 63);
  for (int y = tid >> 6; y < th; y += 4) {
    if (ve >= hw) continue;
    const int4 cw = *reinterpret_cast<const int4*>(&yc[y * 8]);
    const int16_t* b = reinterpret_cast<const int16_t*>(&cw);
    const int r0 = yo[y] - 3 - sy0;
    int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int4 hv = *reinterpret_cast<const int4*>(&hb[min(r0 + k, R - 1) * hs + ve]);
      const int w = b[k];
      v0 += hv.x * w; v1 += hv.y * w; v2 += hv.z * w; v3 += hv.w * w;
    }
    const int phase = (int)((dst_lo + ((uint32_t)(y0 + y) * (uint32_t)p.W2 + (uint32_t)x0) * 3u) & 15u);
    uint8_t* o = &ot[y * RZ_OROW + phase + ve];
    o[0] = (uint8_t)min(max((v0 + (1 << 21)) >> 22, 0), 255);
    if (ve + 1 < hw) o[1] = (uint8_t)min(max((v1 + (1 << 21)) >> 22, 0), 255);
    if (ve + 2 < hw) o[2] = (uint8_t)min(max((v2 + (1 << 21)) >> 22, 0), 255);
    if (ve + 3 < hw) o[3] = (uint8_t)min(max((v3 + (1 << 21)) >> 22, 0), 255);
  }
  __syncthreads();

  // store: per tile row, the 16-byte words that lie wholly inside its destination segment, then the bytes at its two ends
  const int nw = RZ_OROW >> 4;
  for (int i = tid; i < th * nw; i += 256) {
    const int y = i / nw, k = i - y * nw;
    uint8_t* d0 = dst + ((long)(y0 + y) * p.W2 + x0) * 3;
    const int phase = (int)(reinterpret_cast<uintptr_t>(d0) & 15);
    const int lo = 16 * k - phase, hi = lo + 16;                   // the word's bytes relative to the segment start
    if (lo >= 0 && hi <= hw)
      *reinterpret_cast<uint4*>(d0 + lo) = *reinterpret_cast<const uint4*>(&ot[y * RZ_OROW + 16 * k]);
  }
  for (int i = tid; i < th * 32; i += 256) {
    const int y = i >> 5, j = i & 31;
    uint8_t* d0 = dst + ((long)(y0 + y) * p.W2 + x0) * 3;
    const int phase = (int)(reinterpret_cast<uintptr_t>(d0) & 15);
    const int head = min((16 - phase) & 15, hw);                   // bytes before the first whole word
    const int body_end = head + ((hw - head) & ~15);
    const int e = j < 16 ? j : body_end + (j - 16);                // j < 16: head byte j; else tail byte j - 16
    if ((j < 16 && e < head) || (j >= 16 && e < hw)) d0[e] = ot[y * RZ_OROW + phase + e];
  }
}

extern "C" int32_t keep_resize_lanczos4_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2,
                                           int32_t W2, const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs,
                                           const int16_t* ycoef, void* stream) {
  KEEP_REQUIRE(src && dst && xofs && xcoef && yofs && ycoef, "keep_resize_lanczos4_u8: null pointer");
  KEEP_REQUIRE(N > 0 && H > 0 && W > 0 && H2 > 0 && W2 > 0,
               "keep_resize_lanczos4_u8: sizes must be positive (N=%d H=%d W=%d H2=%d W2=%d)", N, H, W, H2, W2);
  KEEP_REQUIRE(W <= INT32_MAX / 3 && W2 <= INT32_MAX / 3, "keep_resize_lanczos4_u8: W * 3 or W2 * 3 overflows int32");
  KEEP_REQUIRE(N <= 65535, "keep_resize_lanczos4_u8: at most 65535 frames per call, got %d", N);
  // tile shape: the largest th, tw (powers of two) whose footprint fits 48 KB of dynamic LDS.  Rows of a tile of th output rows:
  // yofs[y0 + th - 1] - yofs[y0] + 8 <= (th - 1) * H / H2 + 10 (each floor adds at most 1; float rounding of the source
  // coordinate is far below the margin of 3 taken here); the same for columns.
  const double sy = (double)H / H2, sx = (double)W / W2;
  const long lds_cap = 48 << 10;
  int th = RZ_TH, tw = RZ_TW, rcap = 0, srow = 0;
  for (;;) {
    rcap = (int)floor((th - 1) * sy) + 13;
    const long span = (long)floor((tw - 1) * sx) + 13;
    srow = (int)(((span * 3 + 15) + 15) & ~15L);
    const long bytes = (long)rcap * srow + (long)rcap * ((tw * 3 + 3) & ~3) * 4;
    if (bytes <= lds_cap || (th == 1 && tw == 1)) break;
    if (th > 1 && (th >= tw / 2 || tw == 1)) th >>= 1;
    else tw >>= 1;
  }
  const int gx = cdiv(W2, tw), gy = cdiv(H2, th);
  KEEP_REQUIRE(gy <= 65535, "keep_resize_lanczos4_u8: output too tall (H2=%d)", H2);
  ResizeP p;
  p.src = src; p.dst = dst; p.xofs = xofs; p.xcoef = xcoef; p.yofs = yofs; p.ycoef = ycoef;
  p.H = H; p.W = W; p.H2 = H2; p.W2 = W2;
  p.tw = tw; p.th = th; p.rcap = rcap; p.srow = srow;
  p.lg_tw = 0;
  while ((1 << p.lg_tw) < tw) ++p.lg_tw;
  p.hs = (tw * 3 + 3) & ~3;
  const size_t lds = (size_t)rcap * srow + (size_t)rcap * p.hs * 4;
  hipLaunchKernelGGL(resize_lanczos4_u8_kernel, dim3(gx, gy, N), dim3(256), lds, (hipStream_t)stream, p);
  KEEP_LAUNCH_CHECK("keep_resize_lanczos4_u8");
  return KEEP_OK;
}
