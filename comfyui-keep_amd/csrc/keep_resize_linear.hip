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

#include "keep_common.h"
#include "../../include/keep_cv_hip.h"

#pragma clang fp contract(off)

// One block = an output tile of RL_TH rows x RL_TW pixels of one frame (blockIdx.z).  The tile's coefficients -- per column the byte
// offsets of its two source pixels and their weights, per row its two source rows and their weights -- are computed once into LDS: the
// double arithmetic runs once per column and row of a tile.  A thread then produces 4 consecutive pixels of one tile row (16 threads a
// row, 4 rows a wave) into an LDS image of the tile that sits at the byte phase of its destination, and every tile row leaves in
// 16-byte stores (single bytes at its two ends), as in keep_resize_area.hip.
// Source bytes: an output value reads two pixels of two rows whatever the scale.  Where the rectangle between a tile's first and last
// source pixel is small -- enlargements and shrinks up to about 2.5 x, i.e. every face geometry -- it is staged in LDS as the 16-byte
// words that hold it (STAGED; the host passes its capacity, rcap rows of srow bytes).  A larger shrink reads mostly pixels that no
// output uses, so there the threads fetch their 2 x 2 pixels from global memory and nothing is staged: LDS use never grows with the
// span a tile covers.  Every source index is clamped to the frame and, when staged, to the capacity.
#define RL_TW 64
#define RL_TH 16
#define RL_OROW (RL_TW * 3 + 16)       // uint8 output tile row in LDS: 192 bytes + the destination's 16-byte phase
#define RL_FIXED_LDS (RL_TH * RL_OROW + 4 * RL_TW * 4 + 4 * RL_TH * 4)

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
__global__ void __launch_bounds__(256) resize_linear_u8_kernel(LinearP p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rl_dyn[];
  uint8_t* ot = rl_dyn;                                              // [RL_TH][RL_OROW] the output tile
  int* cx0 = reinterpret_cast<int*>(rl_dyn + RL_TH * RL_OROW);       // [RL_TW] byte offset of a column's left source pixel in a (staged) row
  int* cx1 = cx0 + RL_TW;                                            // [RL_TW] ... of its right one
  int* ca0 = cx1 + RL_TW;                                            // [RL_TW] weights of the two, scale 2048
  int* ca1 = ca0 + RL_TW;
  int* ry0 = ca1 + RL_TW;                                            // [RL_TH] the two source rows of a tile row (of the staged rectangle)
  int* ry1 = ry0 + RL_TH;
  int* rb0 = ry1 + RL_TH;                                            // [RL_TH] their weights
  int* rb1 = rb0 + RL_TH;
  uint8_t* sb = rl_dyn + RL_FIXED_LDS;                               // STAGED: [rcap][srow]

  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * RL_TW, y0 = blockIdx.y * RL_TH;
  const int tw = min(RL_TW, p.W2 - x0), th = min(RL_TH, p.H2 - y0);
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

  // (only the low 4 bits of an address matter for a 16-byte phase: 32-bit arithmetic)
  const uint32_t src_lo = (uint32_t)reinterpret_cast<uintptr_t>(src), dst_lo = (uint32_t)reinterpret_cast<uintptr_t>(dst);
  int cx_lo = 0, sy_lo = 0, ncol = p.W, R = p.H;
  if (STAGED) {
    cx_lo = cx0[0];
    sy_lo = ry0[0];
    ncol = min(cx1[tw - 1] - cx_lo + 1, p.ccap);
    R = min(ry1[th - 1] - sy_lo + 1, p.rcap);
    // stage: row r of the rectangle is source row sy_lo + r; its pixels [cx_lo, cx_lo + ncol) as the 16-byte words that hold them
    const int ncol_b = ncol * 3, nchunk = p.srow >> 4;
    for (int i = tid; i < R * nchunk; i += 256) {
      const int r = i / nchunk, k = i - r * nchunk;
      const uint8_t* b0 = src + ((long)(sy_lo + r) * p.W + cx_lo) * 3;
      const uint8_t* a0 = reinterpret_cast<const uint8_t*>(reinterpret_cast<uintptr_t>(b0) & ~(uintptr_t)15);
      // (a word that holds at least one byte of the row segment lies in a page of the buffer: reading all of it cannot fault)
      if (16 * k < (int)(b0 - a0) + ncol_b)
        *reinterpret_cast<uint4*>(sb + (long)r * p.srow + 16 * k) = *reinterpret_cast<const uint4*>(a0 + 16 * k);
    }
    __syncthreads();
  }

  // a thread: 4 consecutive pixels of tile row y
  const int y = tid >> 4, xg = (tid & 15) * 4;
  if (y < th && xg < tw) {
    const int r0 = min(max(ry0[y] - sy_lo, 0), R - 1), r1 = min(max(ry1[y] - sy_lo, 0), R - 1);
    const int b0 = rb0[y], b1 = rb1[y];
    const uint8_t *s0, *s1;
    if (STAGED) {
      s0 = sb + (long)r0 * p.srow + (int)((src_lo + ((uint32_t)(sy_lo + r0) * (uint32_t)p.W + (uint32_t)cx_lo) * 3u) & 15u);
      s1 = sb + (long)r1 * p.srow + (int)((src_lo + ((uint32_t)(sy_lo + r1) * (uint32_t)p.W + (uint32_t)cx_lo) * 3u) & 15u);
    } else {
      s0 = src + (long)r0 * p.W * 3;
      s1 = src + (long)r1 * p.W * 3;
    }
    const int phase = (int)((dst_lo + ((uint32_t)(y0 + y) * (uint32_t)p.W2 + (uint32_t)x0) * 3u) & 15u);
    uint8_t* o = ot + y * RL_OROW + phase + xg * 3;
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

  // store: per tile row, the 16-byte words that lie wholly inside its destination segment, then the bytes at its two ends
  const int hw = tw * 3, nw = RL_OROW >> 4;
  for (int i = tid; i < th * nw; i += 256) {
    const int yy = i / nw, k = i - yy * nw;
    uint8_t* d0 = dst + ((long)(y0 + yy) * p.W2 + x0) * 3;
    const int phase = (int)(reinterpret_cast<uintptr_t>(d0) & 15);
    const int lo = 16 * k - phase, hi = lo + 16;                     // the word's bytes relative to the segment start
    if (lo >= 0 && hi <= hw)
      *reinterpret_cast<uint4*>(d0 + lo) = *reinterpret_cast<const uint4*>(&ot[yy * RL_OROW + 16 * k]);
  }
  for (int i = tid; i < th * 32; i += 256) {
    const int yy = i >> 5, j = i & 31;
    uint8_t* d0 = dst + ((long)(y0 + yy) * p.W2 + x0) * 3;
    const int phase = (int)(reinterpret_cast<uintptr_t>(d0) & 15);
    const int head = min((16 - phase) & 15, hw);                     // bytes before the first whole word
    const int body_end = head + ((hw - head) & ~15);
    const int e = j < 16 ? j : body_end + (j - 16);                  // j < 16: head byte j; else tail byte j - 16
    if ((j < 16 && e < head) || (j >= 16 && e < hw)) d0[e] = ot[yy * RL_OROW + phase + e];
  }
}

// The launch of both entries: `name` opens the error messages; the arguments have been checked for null and non-positive sizes.
static int32_t resize_linear_launch(const char* name, const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2,
                                    int32_t W2, double scale_x, double scale_y, int area2, void* stream) {
  KEEP_REQUIRE(W <= INT32_MAX / 3 && W2 <= INT32_MAX / 3, "%s: W * 3 overflows int32 (W=%d W2=%d)", name, W, W2);
  KEEP_REQUIRE(N <= 65535, "%s: at most 65535 frames per call, got %d", name, N);
  const int gx = cdiv(W2, RL_TW), gy = cdiv(H2, RL_TH);
  KEEP_REQUIRE(gy <= 65535, "%s: output too tall (H2=%d)", name, H2);
  LinearP p;
  p.src = src; p.dst = dst; p.H = H; p.W = W; p.H2 = H2; p.W2 = W2;
  p.scale_x = scale_x;
  p.scale_y = scale_y;
  p.area2 = area2;
  // the rectangle of a tile: its t outputs of an axis are (t - 1) * scale source pixels apart, floor and the right / lower neighbour add
  // two, one more for the float rounding of the coordinates; never more than the frame
  p.rcap = (int)fmin((double)H, floor(RL_TH * p.scale_y) + 4.0);
  p.ccap = (int)fmin((double)W, floor(RL_TW * p.scale_x) + 4.0);
  p.srow = (int)((((long)p.ccap * 3 + 15) + 15) & ~15L);
  const size_t staged = (size_t)p.rcap * (size_t)p.srow;
  if (staged <= (size_t)(24 << 10)) {
    hipLaunchKernelGGL(resize_linear_u8_kernel<true>, dim3(gx, gy, N), dim3(256), RL_FIXED_LDS + staged, (hipStream_t)stream, p);
  } else {
    p.rcap = p.ccap = p.srow = 0;
    hipLaunchKernelGGL(resize_linear_u8_kernel<false>, dim3(gx, gy, N), dim3(256), RL_FIXED_LDS, (hipStream_t)stream, p);
  }
  KEEP_LAUNCH_CHECK(name);
  return KEEP_OK;
}

extern "C" int32_t keep_resize_linear_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2,
                                         void* stream) {
  KEEP_REQUIRE(src && dst, "keep_resize_linear_u8: null pointer");
  KEEP_REQUIRE(N > 0 && H > 0 && W > 0 && H2 > 0 && W2 > 0,
               "keep_resize_linear_u8: sizes must be positive (N=%d H=%d W=%d H2=%d W2=%d)", N, H, W, H2, W2);
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
  KEEP_REQUIRE(src && dst, "keep_resize_linear_fxy_u8: null pointer");
  KEEP_REQUIRE(N > 0 && H > 0 && W > 0 && H2 > 0 && W2 > 0,
               "keep_resize_linear_fxy_u8: sizes must be positive (N=%d H=%d W=%d H2=%d W2=%d)", N, H, W, H2, W2);
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
