// cv2.resize(src uint8 [H,W,3], (W2, H2), interpolation=INTER_LINEAR) on the device, any geometry: the aligned-face input of
// keep_processor.py:158,250 of the reference (frames that are already face crops, brought to 512 x 512).  OpenCV 4.x
// modules/imgproc/src/resize.cpp, two paths:
//   * general: resizeGeneric_ with HResizeLinear<uchar, int, short> / VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>>, the
//     11-bit fixed point that keep_common.h:cv_lin_coef states per axis (columns clamp the position and reset the weight, rows clamp the
//     position and keep the weight); horizontal S0 * a0 + S1 * a1 in int32, vertical
//     (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, saturated.  Identity geometry is an exact copy under this arithmetic.
//   * H == 2 * H2 && W == 2 * W2: cv2.resize turns INTER_LINEAR into INTER_AREA, whose 2 x 2 integer path is (a + b + c + d + 2) >> 2.
// All of it is integer arithmetic behind two double operations per coefficient (rounded separately: __dmul_rn / __dadd_rn, and the
// file is built with FMA contraction off like the other two resizes).  Declared in include/keep_cv_hip.h.
//
// cv2.resize(src, (0, 0), fx=, fy=, interpolation=INTER_LINEAR) -- read_image's enlargement of a frame whose short side is below 512
// (face_restoration_helper.py:182-184) -- is the second entry, keep_resize_linear_fxy_u8: the destination size is the rounded product
// S * f (ties to even), but the coordinate scale is 1.0 / f ITSELF, not recomputed from the rounded size.  Same kernel, same pixel
// arithmetic (rl_value); only the two scales in LinearP differ.  The 2 x 2 substitution cannot occur where a frame is enlarged; the one
// pair of factors at which cv2.resize would make it (a scale of exactly 2 on both axes) is refused, not restated.
#include <math.h>

#include "keep_resize_tile.h"
#include "../../include/keep_cv_hip.h"

#pragma clang fp contract(off)

// One block = an output tile of RL_TH rows x RT_TW pixels of one frame (blockIdx.z).  The tile's coefficients -- per column the byte
// offsets of its two source pixels and their weights, per row its two source rows and their weights -- are computed once into LDS: the
// double arithmetic runs once per column and row of a tile.  A thread then produces 4 consecutive pixels of one tile row (16 threads a
// row, 4 rows a wave) into an LDS image of the tile that sits at the byte phase of its destination, and every tile row leaves in
// 16-byte stores (single bytes at its two ends): the tile I/O of all three resizes, keep_resize_tile.h.
// Source bytes: an output value reads two pixels of two rows whatever the scale.  Where the rectangle between a tile's first and last
// source pixel is small -- enlargements and shrinks up to about 2.5 x, i.e. every face geometry -- it is staged in LDS as the 16-byte
// words that hold it (STAGED; the host passes its capacity, rcap rows of srow bytes).  A larger shrink reads mostly pixels that no
// output uses, so there the threads fetch their 2 x 2 pixels from global memory and nothing is staged: LDS use never grows with the
// span a tile covers.  Every source index is clamped to the frame and, when staged, to the capacity.
#define RL_TH 16
#define RL_FIXED_LDS (RL_TH * RT_OROW + 4 * RT_TW * 4 + 4 * RL_TH * 4)

struct LinearP {
  const uint8_t* src;
  uint8_t* dst;
  int H, W, H2, W2;
  double scale_x, scale_y;             // dsize form: 1. / ((double)W2 / W), 1. / ((double)H2 / H), as OpenCV forms them; fx / fy form: 1. / fx, 1. / fy
  int area2;                           // the exact 2x shrink: (a + b + c + d + 2) >> 2
  int rcap, ccap, srow;                // STAGED: rows / pixels per row / bytes per row of the staged rectangle (capacity)
};

// One output value of both entries from its 2 x 2 source values, the column weights (a0, a1) and the row weights (b0, b1).
__device__ __forceinline__ int rl_value(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1, int area2) {
  if (area2) return (p00 + p01 + p10 + p11 + 2) >> 2;
  const int h0 = p00 * a0 + p01 * a1, h1 = p10 * a0 + p11 * a1;
  return min(255, max(0, (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2));
}

template <bool STAGED>
__global__ void __launch_bounds__(RT_THREADS) resize_linear_u8_kernel(LinearP p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rl_dyn[];
  uint8_t* ot = rl_dyn;                                              // [RL_TH][RT_OROW] the output tile
  int* cx0 = reinterpret_cast<int*>(rl_dyn + RL_TH * RT_OROW);       // [RT_TW] byte offset of a column's left source pixel in a (staged) row
  int* cx1 = cx0 + RT_TW;                                            // [RT_TW] ... of its right one
  int* ca0 = cx1 + RT_TW;                                            // [RT_TW] weights of the two, scale 2048
  int* ca1 = ca0 + RT_TW;
  int* ry0 = ca1 + RT_TW;                                            // [RL_TH] the two source rows of a tile row (of the staged rectangle)
  int* ry1 = ry0 + RL_TH;
  int* rb0 = ry1 + RL_TH;                                            // [RL_TH] their weights
  int* rb1 = rb0 + RL_TH;
  uint8_t* sb = rl_dyn + RL_FIXED_LDS;                               // STAGED: [rcap][srow]

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * RT_TW, y0 = blockIdx.y * RL_TH;
  const int tw = min(RT_TW, p.W2 - x0), th = min(RL_TH, p.H2 - y0);
  const long n = blockIdx.z;
  const uint8_t* src = p.src + n * p.H * (long)p.W * 3;
  uint8_t* dst = p.dst + n * p.H2 * (long)p.W2 * 3;

  // coefficients: absolute source pixels / rows first (monotonic in the destination index: the tile's first and last bound its footprint)
  if (tid < tw) {
    int s, a0, a1, s1;
    if (p.area2) {
      s = 2 * (x0 + tid); s1 = s + 1; a0 = a1 = 0;
    } else {
      cv_lin_coef(x0 + tid, p.scale_x, p.W, true, s, a0, a1);
      s1 = s + 1;
    }
    cx0[tid] = min(max(s, 0), p.W - 1);
    cx1[tid] = min(max(s1, 0), p.W - 1);                             // (a1 = 0 whenever s + 1 is outside)
    ca0[tid] = a0; ca1[tid] = a1;
  } else if (tid >= 64 && tid < 64 + th) {
    const int y = tid - 64;
    int s, b0, b1;
    if (p.area2) {
      s = 2 * (y0 + y); b0 = b1 = 0;
    } else {
      cv_lin_coef(y0 + y, p.scale_y, p.H, false, s, b0, b1);
    }
    ry0[y] = min(max(s, 0), p.H - 1);
    ry1[y] = min(max(s + 1, 0), p.H - 1);
    rb0[y] = b0; rb1[y] = b1;
  }
  __syncthreads();

  int cx_lo = 0, sy_lo = 0, ncol = p.W, R = p.H;
  if (STAGED) {
    cx_lo = cx0[0];
    sy_lo = ry0[0];
    ncol = min(cx1[tw - 1] - cx_lo + 1, p.ccap);
    R = min(ry1[th - 1] - sy_lo + 1, p.rcap);
    // stage: row r of the rectangle is source row sy_lo + r; its pixels [cx_lo, cx_lo + ncol)
    rt_stage(sb, p.srow, src, p.W, cx_lo, ncol * 3, R, [&](int r) { return sy_lo + r; });
    __syncthreads();
  }

  // a thread: 4 consecutive pixels of tile row y
  const int y = tid >> 4, xg = (tid & 15) * 4;
  if (y < th && xg < tw) {
    const int r0 = min(max(ry0[y] - sy_lo, 0), R - 1), r1 = min(max(ry1[y] - sy_lo, 0), R - 1);
    const int b0 = rb0[y], b1 = rb1[y];
    const uint8_t *s0, *s1;
    if (STAGED) {
      s0 = sb + (long)r0 * p.srow + rt_phase(src, sy_lo + r0, p.W, cx_lo);
      s1 = sb + (long)r1 * p.srow + rt_phase(src, sy_lo + r1, p.W, cx_lo);
    } else {
      s0 = src + (long)r0 * p.W * 3;
      s1 = src + (long)r1 * p.W * 3;
    }
    uint8_t* o = ot + y * RT_OROW + rt_phase(dst, y0 + y, p.W2, x0) + xg * 3;
    const int nx = min(4, tw - xg);
    for (int j = 0; j < nx; ++j) {
      const int c0 = min(max(cx0[xg + j] - cx_lo, 0), ncol - 1) * 3, c1 = min(max(cx1[xg + j] - cx_lo, 0), ncol - 1) * 3;
      const int a0 = ca0[xg + j], a1 = ca1[xg + j];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int p00 = s0[c0 + c], p01 = s0[c1 + c], p10 = s1[c0 + c], p11 = s1[c1 + c];
        o[j * 3 + c] = (uint8_t)rl_value(p00, p01, p10, p11, a0, a1, b0, b1, p.area2);
      }
    }
  }
  __syncthreads();

  rt_store_tile(ot, dst, p.W2, x0, y0, th, tw * 3);
}

// The launch of both entries: `name` opens the error messages; the arguments have passed rt_check_args.
static int32_t resize_linear_launch(const char* name, const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2,
                                    int32_t W2, double scale_x, double scale_y, int area2, void* stream) {
  dim3 grid;
  if (int32_t rc = rt_grid(name, N, H2, W2, RL_TH, RT_TW, grid)) return rc;
  LinearP p;
  p.src = src; p.dst = dst; p.H = H; p.W = W; p.H2 = H2; p.W2 = W2;
  p.scale_x = scale_x;
  p.scale_y = scale_y;
  p.area2 = area2;
  // the rectangle of a tile: its t outputs of an axis are (t - 1) * scale source pixels apart, floor and the right / lower neighbour add
  // two, one more for the float rounding of the coordinates; never more than the frame
  p.rcap = (int)fmin((double)H, floor(RL_TH * p.scale_y) + 4.0);
  p.ccap = (int)fmin((double)W, floor(RT_TW * p.scale_x) + 4.0);
  p.srow = (int)((((long)p.ccap * 3 + 15) + 15) & ~15L);
  const size_t staged = (size_t)p.rcap * (size_t)p.srow;
  if (staged <= (size_t)(24 << 10)) {
    hipLaunchKernelGGL(resize_linear_u8_kernel<true>, grid, dim3(RT_THREADS), RL_FIXED_LDS + staged, (hipStream_t)stream, p);
  } else {
    p.rcap = p.ccap = p.srow = 0;
    hipLaunchKernelGGL(resize_linear_u8_kernel<false>, grid, dim3(RT_THREADS), RL_FIXED_LDS, (hipStream_t)stream, p);
  }
  KEEP_LAUNCH_CHECK(name);
  return KEEP_OK;
}

extern "C" int32_t keep_resize_linear_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2,
                                         void* stream) {
  if (int32_t rc = rt_check_args("keep_resize_linear_u8", src && dst, N, H, W, H2, W2)) return rc;
  return resize_linear_launch("keep_resize_linear_u8", src, dst, N, H, W, H2, W2, 1.0 / ((double)W2 / (double)W), 1.0 / ((double)H2 / (double)H),
                              (H == 2 * H2 && W == 2 * W2) ? 1 : 0, stream);
}

// OpenCV's saturate_cast<int>(double): round to nearest, ties to even (lrint under the default rounding mode), saturated.
static inline bool fxy_size(int32_t S, double f, int32_t& D) {
  const double v = nearbyint((double)S * f);
  if (!(v >= 1.0 && v <= (double)INT32_MAX)) return false;
  D = (int32_t)v;
  return true;
}

extern "C" int32_t keep_resize_linear_fxy_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2,
                                             double fx, double fy, void* stream) {
  if (int32_t rc = rt_check_args("keep_resize_linear_fxy_u8", src && dst, N, H, W, H2, W2)) return rc;
  KEEP_REQUIRE(isfinite(fx) && isfinite(fy) && fx > 0.0 && fy > 0.0,
               "keep_resize_linear_fxy_u8: factors must be finite and positive (fx=%g fy=%g)", fx, fy);
  int32_t w2 = 0, h2 = 0;
  KEEP_REQUIRE(fxy_size(W, fx, w2) && fxy_size(H, fy, h2) && w2 == W2 && h2 == H2,
               "keep_resize_linear_fxy_u8: H2 x W2 must be the rounded products H * fy x W * fx (H=%d W=%d fx=%g fy=%g H2=%d W2=%d)", H, W, fx, fy,
               H2, W2);
  KEEP_REQUIRE(!(1.0 / fx == 2.0 && 1.0 / fy == 2.0),
               "keep_resize_linear_fxy_u8: fx = fy = 0.5 is the exact 2x shrink cv2.resize hands to INTER_AREA, which this entry does not restate");
  return resize_linear_launch("keep_resize_linear_fxy_u8", src, dst, N, H, W, H2, W2, 1.0 / fx, 1.0 / fy, 0, stream);
}
