// cv2.resize(src uint8 [H,W,3], (W2, H2), interpolation=INTER_AREA) on the device, shrinking on both axes: the detector input of
// face_restoration_helper.py:206-216.  OpenCV 4.x modules/imgproc/src/resize.cpp (computeResizeAreaTab, ResizeArea_Invoker<uchar,
// float>): per axis a table of (destination, source, weight) entries -- a fractional head, whole source pixels, a fractional tail per
// destination cell, built in double and stored as float -- and per output value a float32 sum over the x entries of every source row
// (buf), folded over the y entries (sum), each multiply and each add rounded on its own.  The order of those operations is the
// arithmetic: this file is built with FMA contraction off (pragma below, Makefile) and the kernel spells them __fmul_rn / __fadd_rn.
// The integer-scale path of OpenCV (is_area_fast) is other arithmetic and is refused here.  Declared in include/keep_cv_hip.h.
#include <float.h>
#include <math.h>

#include "keep_resize_tile.h"
#include "../../include/keep_cv_hip.h"

#pragma clang fp contract(off)

// ---- tables (host C: no device needed) ----------------------------------------------------------------------------------
static inline double area_scale(int S, int D) { return 1.0 / ((double)D / (double)S); }
static inline bool area_scale_is_whole(double scale) { return fabs(scale - (int)scale) < DBL_EPSILON; }

// destination cell d of an axis: whole source pixels [sx1, sx2), a head on sx1 - 1 and a tail on sx2 where their share exceeds 1e-3
struct AreaCell {
  int sx1, sx2;
  bool head, tail;
  double fsx1, fsx2, cell;
};

static inline AreaCell area_cell(int S, double scale, int d) {
  AreaCell c;
  c.fsx1 = d * scale;
  c.fsx2 = c.fsx1 + scale;
  c.cell = fmin(scale, S - c.fsx1);
  int sx1 = (int)ceil(c.fsx1), sx2 = (int)floor(c.fsx2);
  sx2 = sx2 < S - 1 ? sx2 : S - 1;
  sx1 = sx1 < sx2 ? sx1 : sx2;
  c.sx1 = sx1; c.sx2 = sx2;
  c.head = sx1 - c.fsx1 > 1e-3;
  c.tail = c.fsx2 - sx2 > 1e-3;
  return c;
}

static long area_entry_count(int S, int D) {
  const double scale = area_scale(S, D);
  long n = 0;
  for (int d = 0; d < D; ++d) {
    const AreaCell c = area_cell(S, scale, d);
    n += (c.head ? 1 : 0) + (c.sx2 - c.sx1) + (c.tail ? 1 : 0);
  }
  return n;
}

extern "C" int32_t keep_area_tables(int32_t S, int32_t D, int32_t cap, int32_t* start, int32_t* si, float* alpha) {
  KEEP_REQUIRE(start && si && alpha, "keep_area_tables: null pointer");
  KEEP_REQUIRE(S > 0 && D > 0 && cap > 0, "keep_area_tables: sizes must be positive (S=%d, D=%d, cap=%d)", S, D, cap);
  KEEP_REQUIRE(D < S, "keep_area_tables: INTER_AREA tables are for shrinking axes only (S=%d, D=%d)", S, D);
  const long need = area_entry_count(S, D);
  KEEP_REQUIRE(need <= cap, "keep_area_tables: the table of %d -> %d has %ld entries, cap is %d", S, D, need, cap);
  const double scale = area_scale(S, D);
  int k = 0;
  for (int d = 0; d < D; ++d) {
    const AreaCell c = area_cell(S, scale, d);
    start[d] = k;
    if (c.head) {
      si[k] = c.sx1 - 1;
      alpha[k++] = (float)((c.sx1 - c.fsx1) / c.cell);
    }
    for (int sx = c.sx1; sx < c.sx2; ++sx) {
      si[k] = sx;
      alpha[k++] = (float)(1.0 / c.cell);
    }
    if (c.tail) {
      si[k] = c.sx2;
      alpha[k++] = (float)(fmin(fmin(c.fsx2 - c.sx2, 1.0), c.cell) / c.cell);
    }
  }
  start[D] = k;
  return KEEP_OK;
}

// ---- kernel ---------------------------------------------------------------------------------------------------------------
// One block = an output tile of th rows x tw pixels of one frame (blockIdx.z), the shape of the Lanczos kernel (keep_resize.hip).  The
// tile's table entries are copied to LDS with their source indices made relative to the tile's footprint -- source rows
// [ysi[first], ysi[last]], columns [xsi[first], xsi[last]] -- which is staged in LDS with 16-byte loads.  The horizontal pass writes
// buf (float) of every staged row to LDS [rows][tw * 3]: buf depends on the source row and the destination column only, so the
// destination rows that share a source row share it bit for bit.  The vertical pass folds buf over the y entries, rounds, and writes the
// uint8 tile to LDS at the byte phase of its destination; each tile row leaves in 16-byte stores (single bytes at its ends).
// Tap counts are data: the host sizes th / tw / the entry capacities to the scale so that everything fits the dynamic LDS it passes,
// and the kernel clamps every index it reads from a table to those capacities and to the tables' own lengths (xtot / ytot, which the
// launcher recomputes on the host), so tables that are not keep_area_tables' give wrong pixels, never a stray access.
#define RA_TH 32                       // output rows per tile (at most)

struct AreaP {
  const uint8_t* src;
  uint8_t* dst;
  const int32_t* xstart;
  const int32_t* xsi;
  const float* xalpha;
  const int32_t* ystart;
  const int32_t* ysi;
  const float* yalpha;
  int H, W, H2, W2;
  int tw, th, rcap, ccap, srow;        // tile shape; staged source rows / columns (capacity); bytes per staged row
  int lg_tw, hs;                       // log2(tw); float row stride of the horizontal sums (tw * 3 rounded up to 4)
  int xcap, ycap, xtot, ytot;          // entries of a tile per axis (capacity); entries of the whole tables
};

__global__ void __launch_bounds__(RT_THREADS) resize_area_u8_kernel(AreaP p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t ra_dyn[];
  __shared__ int xs[RT_TW + 1], ys[RA_TH + 1];
  __shared__ __attribute__((aligned(16))) uint8_t ot[RA_TH * RT_OROW];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * p.tw, y0 = blockIdx.y * p.th;
  const int tw = min(p.tw, p.W2 - x0), th = min(p.th, p.H2 - y0);
  const long n = blockIdx.z;
  const uint8_t* src = p.src + n * p.H * (long)p.W * 3;
  uint8_t* dst = p.dst + n * p.H2 * (long)p.W2 * 3;

  uint8_t* sb = ra_dyn;                                                   // [rcap][srow] staged source bytes
  float* hb = reinterpret_cast<float*>(ra_dyn + (long)p.rcap * p.srow);  // [rcap][hs] horizontal sums
  int* xcol = reinterpret_cast<int*>(hb + (long)p.rcap * p.hs);          // [xcap] byte offset of an x entry's pixel in a staged row
  float* xa = reinterpret_cast<float*>(xcol + p.xcap);                   // [xcap]
  int* yrow = reinterpret_cast<int*>(xa + p.xcap);                       // [ycap] staged row of a y entry
  float* ya = reinterpret_cast<float*>(yrow + p.ycap);                   // [ycap]

  for (int i = tid; i <= tw; i += 256) xs[i] = min(max(p.xstart[x0 + i], 0), p.xtot);
  for (int i = tid; i <= th; i += 256) ys[i] = min(max(p.ystart[y0 + i], 0), p.ytot);
  __syncthreads();

  // the tile's entries and its source footprint
  const int xe0 = xs[0], ye0 = ys[0];
  const int nxe = min(max(xs[tw] - xe0, 0), p.xcap), nye = min(max(ys[th] - ye0, 0), p.ycap);
  int cx_lo = 0, cx_hi = 0, sy_lo = 0, sy_hi = 0;
  if (nxe > 0) {
    cx_lo = min(max(p.xsi[xe0], 0), p.W - 1);
    cx_hi = min(max(p.xsi[xe0 + nxe - 1], cx_lo), p.W - 1);
  }
  if (nye > 0) {
    sy_lo = min(max(p.ysi[ye0], 0), p.H - 1);
    sy_hi = min(max(p.ysi[ye0 + nye - 1], sy_lo), p.H - 1);
  }
  const int ncol = min(cx_hi - cx_lo + 1, p.ccap), R = min(sy_hi - sy_lo + 1, p.rcap);
  const int ncol_b = ncol * 3;
  for (int i = tid; i < nxe; i += 256) {
    xcol[i] = min(max(p.xsi[xe0 + i] - cx_lo, 0), ncol - 1) * 3;
    xa[i] = p.xalpha[xe0 + i];
  }
  for (int i = tid; i < nye; i += 256) {
    yrow[i] = min(max(p.ysi[ye0 + i] - sy_lo, 0), R - 1);
    ya[i] = p.yalpha[ye0 + i];
  }
  const int hw = tw * 3, hs = p.hs;

  // stage: row r of the footprint is source row sy_lo + r; its columns [cx_lo, cx_lo + ncol)
  rt_stage(sb, p.srow, src, p.W, cx_lo, ncol_b, R, [&](int r) { return sy_lo + r; });
  __syncthreads();

  // horizontal pass: hb[r][x * 3 + c] = buf, the x entries of x in ascending order: buf = buf + (float)src * alpha
  for (int i = tid; i < (R << p.lg_tw); i += 256) {
    const int r = i >> p.lg_tw, x = i & (p.tw - 1);
    if (x >= tw) continue;
    const uint8_t* s = sb + (long)r * p.srow + rt_phase(src, sy_lo + r, p.W, cx_lo);
    const int e0 = min(max(xs[x] - xe0, 0), nxe), e1 = min(max(xs[x + 1] - xe0, e0), nxe);
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    for (int e = e0; e < e1; ++e) {
      const int col = xcol[e];
      const float a = xa[e];
      b0 = __fadd_rn(b0, __fmul_rn((float)s[col], a));
      b1 = __fadd_rn(b1, __fmul_rn((float)s[col + 1], a));
      b2 = __fadd_rn(b2, __fmul_rn((float)s[col + 2], a));
    }
    float* h = hb + r * hs + x * 3;
    h[0] = b0; h[1] = b1; h[2] = b2;
  }
  __syncthreads();

  // vertical pass: sum = beta * buf for the first y entry of the row, sum + beta * buf for the later ones; cvRound, saturate.  A lane
  // owns 4 consecutive bytes of a tile row (16-byte LDS reads), a wave a row
  const int ve = 4 * (tid & 63);
  for (int y = tid >> 6; y < th; y += 4) {
    if (ve >= hw) continue;
    const int e0 = min(max(ys[y] - ye0, 0), nye), e1 = min(max(ys[y + 1] - ye0, e0), nye);
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    for (int e = e0; e < e1; ++e) {
      const float4 hv = *reinterpret_cast<const float4*>(&hb[yrow[e] * hs + ve]);
      const float b = ya[e];
      if (e == e0) {
        v0 = __fmul_rn(b, hv.x); v1 = __fmul_rn(b, hv.y); v2 = __fmul_rn(b, hv.z); v3 = __fmul_rn(b, hv.w);
      } else {
        v0 = __fadd_rn(v0, __fmul_rn(b, hv.x)); v1 = __fadd_rn(v1, __fmul_rn(b, hv.y));
        v2 = __fadd_rn(v2, __fmul_rn(b, hv.z)); v3 = __fadd_rn(v3, __fmul_rn(b, hv.w));
      }
    }
    uint8_t* o = &ot[y * RT_OROW + rt_phase(dst, y0 + y, p.W2, x0) + ve];
    o[0] = (uint8_t)min(max(__float2int_rn(v0), 0), 255);
    if (ve + 1 < hw) o[1] = (uint8_t)min(max(__float2int_rn(v1), 0), 255);
    if (ve + 2 < hw) o[2] = (uint8_t)min(max(__float2int_rn(v2), 0), 255);
    if (ve + 3 < hw) o[3] = (uint8_t)min(max(__float2int_rn(v3), 0), 255);
  }
  __syncthreads();

  rt_store_tile(ot, dst, p.W2, x0, y0, th, hw);
}

extern "C" int32_t keep_resize_area_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2,
                                       const int32_t* xstart, const int32_t* xsi, const float* xalpha, const int32_t* ystart,
                                       const int32_t* ysi, const float* yalpha, void* stream) {
  const char* name = "keep_resize_area_u8";
  if (int32_t rc = rt_check_args(name, src && dst && xstart && xsi && xalpha && ystart && ysi && yalpha, N, H, W, H2, W2)) return rc;
  KEEP_REQUIRE(H2 < H && W2 < W, "keep_resize_area_u8: INTER_AREA is for shrinking on both axes (H=%d W=%d -> H2=%d W2=%d)", H, W, H2, W2);
  const double sy = area_scale(H, H2), sx = area_scale(W, W2);
  KEEP_REQUIRE(!(area_scale_is_whole(sx) && area_scale_is_whole(sy)),
               "keep_resize_area_u8: %dx%d -> %dx%d has a whole-number scale on both axes (OpenCV's integer INTER_AREA path, not restated here)",
               W, H, W2, H2);
  // tile shape: the largest th, tw (powers of two) whose footprint fits 32 KB of dynamic LDS (measured against 48 / 24 / 16 KB at
  // 1080p, 720p and 2160p -> 640 x 1137: 32 and 24 KB are 10-16 % faster than 48 KB, profiles/detect_resize_area.txt).  A tile of th output rows starting at
  // y0 reads source rows ceil(y0 * sy) - 1 .. floor((y0 + th) * sy): at most th * sy + 2, one more taken for the rounding of the
  // products; a destination cell has at most floor(sy) + 3 entries (head, floor(sy) + 1 whole pixels, tail).  The same for columns.
  int th = RA_TH, tw = RT_TW, rcap = 0, ccap = 0, srow = 0, xcap = 0, ycap = 0;
  const auto lds_bytes = [&](int t_h, int t_w) {                     // (leaves the capacities of that tile shape)
    rcap = (int)floor(t_h * sy) + 3;
    ccap = (int)floor(t_w * sx) + 3;
    srow = (int)((((long)ccap * 3 + 15) + 15) & ~15L);
    xcap = t_w * ((int)floor(sx) + 3);
    ycap = t_h * ((int)floor(sy) + 3);
    return (long)rcap * srow + (long)rcap * rt_hs(t_w) * 4 + 8L * (xcap + ycap);
  };
  rt_fit_tile(th, tw, 32 << 10, lds_bytes);
  const size_t lds = (size_t)lds_bytes(th, tw);
  KEEP_REQUIRE(lds <= (size_t)(56 << 10), "keep_resize_area_u8: a one-pixel tile of %dx%d -> %dx%d needs %zu bytes of LDS", W, H, W2, H2, lds);
  dim3 grid;
  if (int32_t rc = rt_grid(name, N, H2, W2, th, tw, grid)) return rc;
  AreaP p;
  p.src = src; p.dst = dst; p.xstart = xstart; p.xsi = xsi; p.xalpha = xalpha; p.ystart = ystart; p.ysi = ysi; p.yalpha = yalpha;
  p.H = H; p.W = W; p.H2 = H2; p.W2 = W2;
  p.tw = tw; p.th = th; p.rcap = rcap; p.ccap = ccap; p.srow = srow;
  p.lg_tw = rt_lg(tw);
  p.hs = rt_hs(tw);
  p.xcap = xcap; p.ycap = ycap;
  p.xtot = (int)area_entry_count(W, W2); p.ytot = (int)area_entry_count(H, H2);
  hipLaunchKernelGGL(resize_area_u8_kernel, grid, dim3(RT_THREADS), lds, (hipStream_t)stream, p);
  KEEP_LAUNCH_CHECK(name);
  return KEEP_OK;
}
