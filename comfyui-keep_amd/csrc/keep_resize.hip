// cv2.resize(src uint8 [H,W,3], (W2, H2), interpolation=INTER_LANCZOS4) on the device: the background resize of
// final_upscale_factor (face_restoration_helper.py:354-356, keep_processor.py:139-142,283-286 of the reference).
// OpenCV 4.x modules/imgproc/src/resize.cpp (resizeGeneric_, HResizeLanczos4<uchar,int,short,2048>, VResizeLanczos4 with
// FixedPtCast<int,uchar,22>, interpolateLanczos4): per axis a table of 8 int16 coefficients (scale 2048) and one source
// offset per destination index; tap i of destination d reads source clamp(ofs[d] - 3 + i, 0, S - 1).  Both passes are exact
// int32 sums, so their order does not matter: the tables are the only delicate part, and they are built on the host
// (keep_lanczos4_tables) with OpenCV's own double / float operation sequence, FMA contraction off (Makefile).
#include <math.h>

#include "keep_resize_tile.h"

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
#define RZ_TH 32                       // output rows per tile (at most)

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

__global__ void __launch_bounds__(RT_THREADS) resize_lanczos4_u8_kernel(ResizeP p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rz_dyn[];
  __shared__ int xo[RT_TW], yo[RZ_TH];
  __shared__ __attribute__((aligned(16))) int16_t xc[RT_TW * 8], yc[RZ_TH * 8];
  __shared__ __attribute__((aligned(16))) uint8_t ot[RZ_TH * RT_OROW];
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

  // stage: row r of the footprint is source row clamp(sy0 + r); its columns [cx_lo, cx_hi]
  const auto row_of = [&](int r) { return min(max(sy0 + r, 0), p.H - 1); };
  rt_stage(sb, p.srow, src, p.W, cx_lo, ncol_b, R, row_of);
  __syncthreads();

  // horizontal pass: hb[r][x * 3 + c] = sum_i src[row][clamp(xofs[x] - 3 + i)][c] * xcoef[x][i]
  for (int i = tid; i < (R << p.lg_tw); i += 256) {
    const int r = i >> p.lg_tw, x = i & (p.tw - 1);
    if (x >= tw) continue;
    const uint8_t* s = sb + (long)r * p.srow + rt_phase(src, row_of(r), p.W, cx_lo);
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
    uint8_t* o = &ot[y * RT_OROW + rt_phase(dst, y0 + y, p.W2, x0) + ve];
    o[0] = (uint8_t)min(max((v0 + (1 << 21)) >> 22, 0), 255);
    if (ve + 1 < hw) o[1] = (uint8_t)min(max((v1 + (1 << 21)) >> 22, 0), 255);
    if (ve + 2 < hw) o[2] = (uint8_t)min(max((v2 + (1 << 21)) >> 22, 0), 255);
    if (ve + 3 < hw) o[3] = (uint8_t)min(max((v3 + (1 << 21)) >> 22, 0), 255);
  }
  __syncthreads();

  rt_store_tile(ot, dst, p.W2, x0, y0, th, hw);
}

extern "C" int32_t keep_resize_lanczos4_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2,
                                           int32_t W2, const int32_t* xofs, const int16_t* xcoef, const int32_t* yofs,
                                           const int16_t* ycoef, void* stream) {
  const char* name = "keep_resize_lanczos4_u8";
  if (int32_t rc = rt_check_args(name, src && dst && xofs && xcoef && yofs && ycoef, N, H, W, H2, W2)) return rc;
  // tile shape: the largest th, tw (powers of two) whose footprint fits 48 KB of dynamic LDS.  Rows of a tile of th output rows:
  // yofs[y0 + th - 1] - yofs[y0] + 8 <= (th - 1) * H / H2 + 10 (each floor adds at most 1; float rounding of the source
  // coordinate is far below the margin of 3 taken here); the same for columns.
  const double sy = (double)H / H2, sx = (double)W / W2;
  int th = RZ_TH, tw = RT_TW, rcap = 0, srow = 0;
  const auto lds_bytes = [&](int t_h, int t_w) {                     // (leaves rcap / srow of that tile shape)
    rcap = (int)floor((t_h - 1) * sy) + 13;
    const long span = (long)floor((t_w - 1) * sx) + 13;
    srow = (int)(((span * 3 + 15) + 15) & ~15L);
    return (long)rcap * srow + (long)rcap * rt_hs(t_w) * 4;
  };
  rt_fit_tile(th, tw, 48 << 10, lds_bytes);
  dim3 grid;
  if (int32_t rc = rt_grid(name, N, H2, W2, th, tw, grid)) return rc;
  ResizeP p;
  p.src = src; p.dst = dst; p.xofs = xofs; p.xcoef = xcoef; p.yofs = yofs; p.ycoef = ycoef;
  p.H = H; p.W = W; p.H2 = H2; p.W2 = W2;
  p.tw = tw; p.th = th; p.rcap = rcap; p.srow = srow;
  p.lg_tw = rt_lg(tw);
  p.hs = rt_hs(tw);
  hipLaunchKernelGGL(resize_lanczos4_u8_kernel, grid, dim3(RT_THREADS), (size_t)lds_bytes(th, tw), (hipStream_t)stream, p);
  KEEP_LAUNCH_CHECK(name);
  return KEEP_OK;
}
