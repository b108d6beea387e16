// Tone match of restored faces (engine/tone.py; tests/tone_match_ref.py restates it in numpy, bit for bit): the low spatial band of the
// source crop replaces the restored face's,  out = rst + lowpass(src - rst),  a separable Gaussian in integers throughout.  Per channel,
// indices clamped at the borders, taps t[-R .. R] >= 0 with sum 4096 (validated by the launcher: every int32 bound below rests on it):
//     d  = src - rst                                  [-255, 255]
//     hh = sum_k t[k] * d[y, clamp(x + k)]            |hh| <= 255 * 4096
//     h4 = (hh + 128) >> 8                            |h4| <= 4080: int16, 4 fractional bits
//     v  = sum_k t[k] * h4[clamp(y + k), x]           |v| <= 4080 * 4096 < 2^24
//     out = clamp(rst + ((v + 32768) >> 16), 0, 255)
// No float and no atomic anywhere: the result depends neither on the summation order, the launch geometry nor the batch.
// Declared in include/keep_cv_hip.h.
//
// Two passes with the int16 h4 image in the caller's scratch.  The scratch layout is the library's own: PLANAR, [F][3][h][w], so that a lane
// of pass 1 stores 8 consecutive values as 16 bytes and pass 2 stages plain rows.
//
// Both inner products are int16 x int16 -> int32 dot products of PAIRS (v_dot2c_i32_i16): a register holds two neighbouring samples of the
// filtered axis at an EVEN position, and a lane computes 8 consecutive outputs o .. o + 7 from the pair stream P[j] = (s[o + 2j], s[o + 2j + 1]):
//     out[o + 2q]     = sum_m  Te[m] . P[m + q]        Te[m] = (T[2m], T[2m + 1])          T[i] = t[i - Rp], 0 outside -R .. R
//     out[o + 2q + 1] = sum_m  To[m] . P[m + q]        To[m] = (T[2m - 1], T[2m])          the same taps one sample later
// with Rp = R rounded up to even, so that the window of an even output starts at an even sample.  One pair register feeds 8 dot products;
// the two tap sets (np4 = Rp + 1 rounded up to 4 pairs each, zero padded) travel in the kernel arguments and are read into SGPRs.
//
// Pass 1 (256 threads = 8 rows x 256 pixels): src and rst are read once in groups of 4 pixels (12 bytes as they lie; groups that touch
// a border pixel by pixel with the clamp), d goes to LDS de-interleaved into three channel planes, so a lane's pairs are 16 contiguous
// bytes per step (ds_read_b128, lanes contiguous: conflict-free).  Pass 2 (384 threads = 32 rows x 64 columns x 3 planes): the h4 rows
// Y0 - Rp .. of the tile are staged as they lie; a lane takes two neighbouring columns, reads one dword per row (32 lanes = one contiguous
// row segment: conflict-free) and packs the rows pairwise.  The deltas meet in LDS channel-interleaved, and rst / out move 12 bytes at a time.
#include <string.h>

#include "keep_common.h"
#include "../../include/keep_cv_hip.h"

#define TN_RMAX 128
#define TN_NPMAX 132                    // pairs per tap set: (Rp + 1) rounded up to 4, Rp <= 128
#define TN1_THREADS 256
#define TN1_TW 256                      // pass 1: pixels per tile row
#define TN1_TH 8                        //         rows per tile
#define TN1_LMAX (TN1_TW + 2 * TN_NPMAX)
#define TN2_THREADS 384                 // one lane per task: 3 planes x 32 column pairs x 4 groups of 8 rows
#define TN2_TC 64                       // pass 2: columns per tile
#define TN2_TR 32                       //         rows per tile

typedef short tn_s2 __attribute__((ext_vector_type(2)));

struct ToneP {
  const uint8_t* src;
  const uint8_t* rst;
  uint8_t* out;
  int16_t* scratch;
  int h, w;
  int Rp, np4;                          // R rounded up to even; pairs per tap set
  int tx, ty;                           // tiles per face along x / y (of the pass launched)
  int wide;                             // w % 8 == 0 and scratch 16-byte aligned: h4 rows move 16 bytes at a time
  uint32_t te[TN_NPMAX], to[TN_NPMAX];  // the tap pairs of even / odd outputs, low half = the earlier sample
};

__device__ __forceinline__ int tn_dot(uint32_t a, uint32_t t, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(tn_s2, a), __builtin_bit_cast(tn_s2, t), acc, false);
}

// one step of the 8-output filter: pairs a0 .. a3 = P[m] .. P[m + 3]
__device__ __forceinline__ void tn_step(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t te, uint32_t to, int (&acc)[8]) {
  acc[0] = tn_dot(a0, te, acc[0]); acc[1] = tn_dot(a0, to, acc[1]);
  acc[2] = tn_dot(a1, te, acc[2]); acc[3] = tn_dot(a1, to, acc[3]);
  acc[4] = tn_dot(a2, te, acc[4]); acc[5] = tn_dot(a2, to, acc[5]);
  acc[6] = tn_dot(a3, te, acc[6]); acc[7] = tn_dot(a3, to, acc[7]);
}

__device__ __forceinline__ int tn_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- pass 1: d = src - rst, filtered along x, rounded to 4 fractional bits -> scratch (planar)
__global__ void __launch_bounds__(TN1_THREADS) tone_h_kernel(ToneP p) {
  __shared__ __attribute__((aligned(16))) int16_t sd[3 * TN1_TH * TN1_LMAX];
  const int tid = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  const int bx = (int)(blk % (uint32_t)p.tx);
  const int by = (int)((blk / (uint32_t)p.tx) % (uint32_t)p.ty);
  const long f = blk / ((uint32_t)p.tx * (uint32_t)p.ty);
  const int X0 = bx * TN1_TW, Y0 = by * TN1_TH;
  const int L = TN1_TW + 2 * p.np4;     // staged samples per row (a multiple of 8); sample 0 is pixel X0 - Rp
  const int gpr = L >> 2;               // groups of 4 pixels per staged row
  const int rows = min(TN1_TH, p.h - Y0);
  const long face = f * ((long)p.h * p.w * 3);

  for (int i = tid; i < rows * gpr; i += TN1_THREADS) {
    const int row = i / gpr, g = i - row * gpr;
    const int xa = X0 - p.Rp + 4 * g;
    const long rowoff = face + (long)(Y0 + row) * p.w * 3;
    uint8_t s[12], r[12];
    if (xa >= 0 && xa + 4 <= p.w) {
      memcpy(s, p.src + rowoff + (long)xa * 3, 12);
      memcpy(r, p.rst + rowoff + (long)xa * 3, 12);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long o = rowoff + (long)tn_clampi(xa + j, 0, p.w - 1) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          s[3 * j + c] = p.src[o + c];
          r[3 * j + c] = p.rst[o + c];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int16_t d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) d[j] = (int16_t)((int)s[3 * j + c] - (int)r[3 * j + c]);
      memcpy(sd + (c * TN1_TH + row) * L + 4 * g, d, 8);
    }
  }
  __syncthreads();

  for (int t = tid; t < rows * (3 * TN1_TW / 8); t += TN1_THREADS) {
    const int g = t % (TN1_TW / 8), c = (t / (TN1_TW / 8)) % 3, row = t / (3 * TN1_TW / 8);
    const int x = X0 + 8 * g;
    if (x >= p.w) continue;
    const uint4* q = reinterpret_cast<const uint4*>(sd + (c * TN1_TH + row) * L + 8 * g);
    int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint4 a = q[0];
    for (int m = 0; m < p.np4; m += 4) {
      const uint4 b = q[(m >> 2) + 1];
      tn_step(a.x, a.y, a.z, a.w, p.te[m], p.to[m], acc);
      tn_step(a.y, a.z, a.w, b.x, p.te[m + 1], p.to[m + 1], acc);
      tn_step(a.z, a.w, b.x, b.y, p.te[m + 2], p.to[m + 2], acc);
      tn_step(a.w, b.x, b.y, b.z, p.te[m + 3], p.to[m + 3], acc);
      a = b;
    }
    int16_t h4[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) h4[j] = (int16_t)((acc[j] + 128) >> 8);
    int16_t* dst = p.scratch + ((f * 3 + c) * (long)p.h + (Y0 + row)) * p.w + x;
    if (p.wide) {
      uint4 v;
      memcpy(&v, h4, 16);
      *reinterpret_cast<uint4*>(dst) = v;
    } else {
      const int n = min(8, p.w - x);
      for (int j = 0; j < n; ++j) dst[j] = h4[j];
    }
  }
}

// ---- pass 2: h4 filtered along y, rounded, added to rst -> out
__global__ void __launch_bounds__(TN2_THREADS) tone_v_kernel(ToneP p) {
  extern __shared__ __attribute__((aligned(16))) int16_t sh[];   // [3][NR][TN2_TC]; afterwards the deltas [TN2_TR][TN2_TC * 3]
  const int tid = threadIdx.x;
  const uint32_t blk = blockIdx.x;
  const int bx = (int)(blk % (uint32_t)p.tx);
  const int by = (int)((blk / (uint32_t)p.tx) % (uint32_t)p.ty);
  const long f = blk / ((uint32_t)p.tx * (uint32_t)p.ty);
  const int X0 = bx * TN2_TC, Y0 = by * TN2_TR;
  const int NR = TN2_TR + 2 * p.np4;    // staged rows; row 0 is image row Y0 - Rp

  for (int i = tid; i < 3 * NR * (TN2_TC / 8); i += TN2_THREADS) {
    const int j = i % (TN2_TC / 8), rr = (i / (TN2_TC / 8)) % NR, pl = i / ((TN2_TC / 8) * NR);
    const int yy = tn_clampi(Y0 - p.Rp + rr, 0, p.h - 1);
    const int x = X0 + 8 * j;
    const int16_t* srow = p.scratch + ((f * 3 + pl) * (long)p.h + yy) * p.w;
    uint4 v;
    if (p.wide && x + 8 <= p.w) {
      v = *reinterpret_cast<const uint4*>(srow + x);
    } else {
      int16_t e[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) e[k] = srow[min(x + k, p.w - 1)];   // (columns past the image feed outputs nobody writes)
      memcpy(&v, e, 16);
    }
    *reinterpret_cast<uint4*>(sh + (pl * NR + rr) * TN2_TC + 8 * j) = v;
  }
  __syncthreads();

  // a lane's task: two neighbouring columns of one plane, 8 rows
  static_assert(3 * (TN2_TC / 2) * (TN2_TR / 8) == TN2_THREADS, "one task per lane");
  const int cp = tid % (TN2_TC / 2), pl = (tid / (TN2_TC / 2)) % 3, rg = tid / (3 * TN2_TC / 2);
  int16_t dl[16];
  {
    const uint32_t* col = reinterpret_cast<const uint32_t*>(sh + (pl * NR + 8 * rg) * TN2_TC) + cp;
    int accA[8] = {0, 0, 0, 0, 0, 0, 0, 0}, accB[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t A[7], B[7];                // pairs of rows of column 2 cp (A) and 2 cp + 1 (B)
#define TN_LOADPAIR(i, j)                                                      \
  do {                                                                         \
    const uint32_t w0 = col[(2 * (j)) * (TN2_TC / 2)], w1 = col[(2 * (j) + 1) * (TN2_TC / 2)]; \
    A[i] = (w0 & 0xffffu) | (w1 << 16);                                        \
    B[i] = (w0 >> 16) | (w1 & 0xffff0000u);                                    \
  } while (0)
    TN_LOADPAIR(0, 0); TN_LOADPAIR(1, 1); TN_LOADPAIR(2, 2); TN_LOADPAIR(3, 3);
    for (int m = 0; m < p.np4; m += 4) {
      TN_LOADPAIR(4, m + 4); TN_LOADPAIR(5, m + 5); TN_LOADPAIR(6, m + 6);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        tn_step(A[s], A[s + 1], A[s + 2], A[s + 3], p.te[m + s], p.to[m + s], accA);
        tn_step(B[s], B[s + 1], B[s + 2], B[s + 3], p.te[m + s], p.to[m + s], accB);
      }
      A[0] = A[4]; A[1] = A[5]; A[2] = A[6];
      B[0] = B[4]; B[1] = B[5]; B[2] = B[6];
      if (m + 4 < p.np4) TN_LOADPAIR(3, m + 7);
    }
#undef TN_LOADPAIR
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dl[j] = (int16_t)((accA[j] + 32768) >> 16);
      dl[8 + j] = (int16_t)((accB[j] + 32768) >> 16);
    }
  }
  __syncthreads();                      // every lane has read its rows: the staging area becomes the delta tile
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sh[(8 * rg + j) * (TN2_TC * 3) + (2 * cp) * 3 + pl] = dl[j];
    sh[(8 * rg + j) * (TN2_TC * 3) + (2 * cp + 1) * 3 + pl] = dl[8 + j];
  }
  __syncthreads();

  const long face = f * ((long)p.h * p.w * 3);
  for (int i = tid; i < TN2_TR * (TN2_TC / 4); i += TN2_THREADS) {
    const int g = i % (TN2_TC / 4), row = i / (TN2_TC / 4);
    const int x = X0 + 4 * g, y = Y0 + row;
    if (y >= p.h || x >= p.w) continue;
    const long o = face + ((long)y * p.w + x) * 3;
    int16_t d[12];
    memcpy(d, sh + row * (TN2_TC * 3) + 12 * g, 24);
    if (x + 4 <= p.w) {
      uint8_t r[12], q[12];
      memcpy(r, p.rst + o, 12);
#pragma unroll
      for (int j = 0; j < 12; ++j) q[j] = (uint8_t)tn_clampi((int)r[j] + (int)d[j], 0, 255);
      memcpy(p.out + o, q, 12);
    } else {
      const int n = 3 * (p.w - x);
      for (int j = 0; j < n; ++j) p.out[o + j] = (uint8_t)tn_clampi((int)p.rst[o + j] + (int)d[j], 0, 255);
    }
  }
}

static bool tn_overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

extern "C" int32_t keep_tone_match_u8(const uint8_t* src, const uint8_t* rst, uint8_t* out, int16_t* scratch, int32_t F, int32_t h,
                                      int32_t w, const int16_t* taps, int32_t R, void* stream) {
  KEEP_REQUIRE(src && rst && out && scratch && taps, "keep_tone_match_u8: null pointer");
  KEEP_REQUIRE(F > 0 && h > 0 && w > 0, "keep_tone_match_u8: sizes must be positive (F=%d h=%d w=%d)", F, h, w);
  KEEP_REQUIRE(h < 32768 && w < 32768, "keep_tone_match_u8: h and w must be below 32768 (h=%d w=%d)", h, w);
  KEEP_REQUIRE(R >= 1 && R <= TN_RMAX, "keep_tone_match_u8: R must be in 1 .. %d (R=%d)", TN_RMAX, R);
  long sum = 0;
  for (int i = 0; i <= 2 * R; ++i) {
    KEEP_REQUIRE(taps[i] >= 0, "keep_tone_match_u8: tap %d is negative (%d)", i - R, (int)taps[i]);
    sum += taps[i];
  }
  KEEP_REQUIRE(sum == 4096, "keep_tone_match_u8: the taps must sum to 4096 (sum=%ld)", sum);
  // a block reads its neighbours' src and rst through the halo, and pass 2 reads what pass 1 wrote: nothing written may alias anything read
  const int64_t n = (int64_t)F * h * w * 3;
  KEEP_REQUIRE(!tn_overlap(out, n, src, n) && !tn_overlap(out, n, rst, n), "keep_tone_match_u8: out overlaps src or rst (in place is a race)");
  KEEP_REQUIRE(!tn_overlap(scratch, 2 * n, src, n) && !tn_overlap(scratch, 2 * n, rst, n), "keep_tone_match_u8: scratch overlaps src or rst");
  KEEP_REQUIRE(!tn_overlap(scratch, 2 * n, out, n), "keep_tone_match_u8: scratch overlaps out");

  ToneP p;
  memset(&p, 0, sizeof(p));
  p.h = h; p.w = w;
  p.Rp = R + (R & 1);
  p.np4 = (p.Rp + 1 + 3) & ~3;
  p.wide = (w % 8 == 0) && ((uintptr_t)scratch % 16 == 0);
  {
    int16_t T[2 * TN_NPMAX + 1];        // T[1 + i] = t[i - Rp]; T[0] = 0 is the sample in front of an odd output's window
    memset(T, 0, sizeof(T));
    for (int k = -R; k <= R; ++k) T[1 + p.Rp + k] = taps[R + k];
    for (int m = 0; m < p.np4; ++m) {
      p.te[m] = (uint32_t)(uint16_t)T[1 + 2 * m] | ((uint32_t)(uint16_t)T[2 + 2 * m] << 16);
      p.to[m] = (uint32_t)(uint16_t)T[2 * m] | ((uint32_t)(uint16_t)T[1 + 2 * m] << 16);
    }
  }
  const size_t lds2 = (size_t)3 * (TN2_TR + 2 * p.np4) * TN2_TC * sizeof(int16_t);   // <= 113,664 bytes (>= the 12,288 of the delta tile)
  if (int rc = keep_raise_lds_limit<tone_v_kernel>("keep_tone_match_u8")) return rc;

  hipStream_t st = (hipStream_t)stream;
  const int tx1 = cdiv(w, TN1_TW), ty1 = cdiv(h, TN1_TH);
  const int tx2 = cdiv(w, TN2_TC), ty2 = cdiv(h, TN2_TR);
  const long per1 = (long)tx1 * ty1, per2 = (long)tx2 * ty2;     // < 2^19 each
  const long cap = (1L << 30) / (per1 > per2 ? per1 : per2);     // faces per launch: the grid's x extent stays below 2^31
  for (long f0 = 0; f0 < F; f0 += cap) {
    const long m = F - f0 < cap ? F - f0 : cap;
    const long off = f0 * ((long)h * w * 3);
    p.src = src + off; p.rst = rst + off; p.out = out + off; p.scratch = scratch + off;
    p.tx = tx1; p.ty = ty1;
    hipLaunchKernelGGL(tone_h_kernel, dim3((unsigned)(m * per1)), dim3(TN1_THREADS), 0, st, p);
    p.tx = tx2; p.ty = ty2;
    hipLaunchKernelGGL(tone_v_kernel, dim3((unsigned)(m * per2)), dim3(TN2_THREADS), lds2, st, p);
  }
  KEEP_LAUNCH_CHECK("keep_tone_match_u8");
  return KEEP_OK;
}
