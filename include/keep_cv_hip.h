/* keep_cv_hip.h -- extension header of libkeep_hip.so: OpenCV-arithmetic image kernels that are not part of the core C-ABI.
 *
 * The core header (keep_hip.h) and its KEEP_ABI_VERSION are frozen; entry points added beside it live here under a version of their
 * own, in the same shared library.  The boundary rules are the core header's:
 *   - every pointer the caller passes is CALLER-OWNED; device pointers are plain device memory (torch tensor.data_ptr() works);
 *   - launchers are stream-ordered on the hipStream_t passed as `void* stream` (NULL = default stream), allocate nothing and
 *     synchronise nothing;
 *   - returns KEEP_OK (0), KEEP_EINVAL (-1) bad argument / refused geometry, KEEP_EHIP (-3) HIP runtime error, with a thread-local
 *     message behind keep_hip.h's keep_last_error that opens with the function's name;
 *   - the library reads no environment variable.
 */
#ifndef KEEP_CV_HIP_H
#define KEEP_CV_HIP_H

#include <stdint.h>

#include "keep_hip.h" /* keep_attention_args */

#ifdef __cplusplus
extern "C" {
#endif

#define KEEP_CV_ABI_VERSION 1

int32_t keep_cv_abi_version(void);

/* ---- detector input (face_restoration_helper.py:206-216): cv2.resize(frame, (W2, H2), interpolation=INTER_AREA), uint8, 3 channels,
 * shrinking on BOTH axes: OpenCV 4.x resize.cpp computeResizeAreaTab + ResizeArea_Invoker<uchar, float>.
 *
 * Refused geometries (KEEP_EINVAL): D >= S on an axis, and -- by the launcher -- a geometry whose scale 1.0 / ((double)D / S) is a
 * whole number on BOTH axes (OpenCV's is_area_fast: an integer path with other arithmetic, which this library does not restate).
 *
 * keep_area_tables: HOST-only C (no device, no stream): the table of one axis, S source -> D destination pixels, in CSR form: the
 * entries of destination index d are start[d] .. start[d + 1] - 1, entry e adds source pixel si[e] with weight alpha[e], source indices
 * ascending.  start has D + 1 elements, si / alpha have `cap` elements; KEEP_EINVAL when the table needs more than `cap` entries (an axis
 * never needs more than S + 2 * D).
 *
 * keep_resize_area_u8: N contiguous uint8 frames [N,H,W,3] -> [N,H2,W2,3] in one launch with the tables of x (W -> W2) and y
 * (H -> H2) as keep_area_tables wrote them, all DEVICE pointers.  Per output value, in float32 with separately rounded multiplies and
 * adds: for every y entry in order, buf = sum over the x entries in order of src * alpha; sum = beta * buf for the first y entry,
 * sum + beta * buf for the later ones; dst = saturate_u8(round-half-to-even(sum)). */
int32_t keep_area_tables(int32_t S, int32_t D, int32_t cap, int32_t* start /*[D+1]*/, int32_t* si /*[cap]*/, float* alpha /*[cap]*/);
int32_t keep_resize_area_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2,
                            const int32_t* xstart, const int32_t* xsi, const float* xalpha, const int32_t* ystart, const int32_t* ysi,
                            const float* yalpha, void* stream);

/* ---- aligned-face input (keep_processor.py:158,250 of the reference): cv2.resize(frame, (W2, H2), interpolation=INTER_LINEAR), uint8,
 * 3 channels, ANY geometry (enlarging, shrinking, mixed; identity is an exact copy): OpenCV 4.x resize.cpp.
 *
 * keep_resize_linear_u8: N contiguous uint8 frames [N,H,W,3] -> [N,H2,W2,3] in one launch, DEVICE pointers, no tables.  Per axis
 * scale = 1.0 / ((double)D / S); f = (float)((d + 0.5) * scale - 0.5), product and sum rounded separately in double; s = floor(f),
 * f -= s; columns: s < 0 -> (0, f = 0), s >= S - 1 -> (S - 1, f = 0); rows are clamped to [0, S - 1] and keep their weights; weights
 * sat_short(rint((1.f - f) * 2048)), sat_short(rint(f * 2048)); horizontal S0 * a0 + S1 * a1 in int32; vertical
 * (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2, saturated to 0..255.  H == 2 * H2 && W == 2 * W2 is the case
 * cv2.resize hands to INTER_AREA's 2 x 2 integer path: (a + b + c + d + 2) >> 2 per channel. */
int32_t keep_resize_linear_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2, void* stream);

/* ---- read_image's enlargement of a small frame (face_restoration_helper.py:182-184): cv2.resize(frame, (0, 0), fx=fx, fy=fy,
 * interpolation=INTER_LINEAR), uint8, 3 channels -- the form of cv2.resize with an empty dsize.
 *
 * keep_resize_linear_fxy_u8: as keep_resize_linear_u8 (one launch, DEVICE pointers, no tables, the same kernel and pixel arithmetic) with
 * two differences: the per-axis scale is 1.0 / fx (1.0 / fy) ITSELF, not recomputed from the sizes, and there is no 2 x 2 substitution: an
 * enlargement never meets it, and the one pair of factors at which cv2.resize makes it (1.0 / fx == 2 && 1.0 / fy == 2) is refused.  The
 * caller passes the destination size OpenCV computes, W2 = saturate_cast<int>(W * fx), H2 = saturate_cast<int>(H * fy): round to nearest,
 * ties to even.  KEEP_EINVAL, before anything is launched: a null pointer; N, H, W, H2 or W2 <= 0; a factor that is not finite or not
 * positive; H2 / W2 other than those rounded products; fx == fy == 0.5; and the size limits of keep_resize_linear_u8. */
int32_t keep_resize_linear_fxy_u8(const uint8_t* src, uint8_t* dst, int32_t N, int32_t H, int32_t W, int32_t H2, int32_t W2, double fx,
                                  double fy, void* stream);

/* ---- the aligned crops of a chunk of frames (face_restoration_helper.py:316-318): cv2.warpAffine(frame, M, (dw, dh), INTER_LINEAR,
 * BORDER_CONSTANT, borderValue) for F faces taken from N resident frames, uint8, 3 channels -- per pixel the arithmetic of keep_hip.h's
 * single-frame crop warp (one shared device function): 1/1024 fixed-point coordinates from separately rounded double multiplies, 5-bit
 * fractions, 15-bit weights, the border colour for taps outside the source.
 *
 * keep_warp_affine_batch_u8: `frames` [N,H,W,3] and `dst` [F,dh,dw,3] are contiguous DEVICE memory; `frame_of` [F] and `dst_to_src` [F*6]
 * (the destination -> source map of face f, row-major 2 x 3) are HOST arrays, read before the call returns: they travel in the kernel
 * arguments, at most 32 faces per launch, so F faces are ceil(F / 32) launches on `stream`.  frame_of[f] == -1 writes a black crop (the
 * `None` matrix of align_warp_face, :309-311); its matrix is not used but must be finite.  KEEP_EINVAL, before anything is launched: a null
 * pointer; N, F, H, W, dh or dw <= 0; H or W >= 32768; a frame index outside -1 .. N - 1; a non-finite matrix entry.
 *
 * keep_warp_batch_group: HOST-only C (no device, no stream): launch g of F faces covers faces first .. first + count - 1 -- the rule the
 * launcher itself loops over; KEEP_EINVAL for a g that F faces have no launch for.
 *
 * keep_warp_affine_batch_scatter_u8: the same warp (the same kernel, launches and pixel arithmetic) with every face written to a slot of
 * the caller's choosing: `dst` is [n_slots,dh,dw,3] and face f goes to dst + slot_of[f] * dh * dw * 3; `slot_of` [F] is a HOST array like
 * `frame_of`.  A slot no face names is not written.  KEEP_EINVAL, before anything is launched: everything keep_warp_affine_batch_u8
 * refuses; n_slots < F; a slot outside 0 .. n_slots - 1; a slot named twice. */
int32_t keep_warp_batch_group(int32_t F, int32_t g, int32_t* first, int32_t* count);
int32_t keep_warp_affine_batch_u8(const uint8_t* frames, int32_t N, int32_t H, int32_t W, uint8_t* dst, int32_t F, int32_t dh, int32_t dw,
                                  const int32_t* frame_of /*host [F]*/, const double* dst_to_src /*host [F*6]*/, int32_t border_b,
                                  int32_t border_g, int32_t border_r, void* stream);
int32_t keep_warp_affine_batch_scatter_u8(const uint8_t* frames, int32_t N, int32_t H, int32_t W, uint8_t* dst, int32_t n_slots, int32_t F,
                                          int32_t dh, int32_t dw, const int32_t* frame_of /*host [F]*/, const int32_t* slot_of /*host [F]*/,
                                          const double* dst_to_src /*host [F*6]*/, int32_t border_b, int32_t border_g, int32_t border_r,
                                          void* stream);

/* ---- what one attention call of keep_hip.h would launch: HOST-only C (no device, no stream; no pointer of `a` is dereferenced, they are
 * tested for alignment only, so aligned made-up addresses do).  The arguments go through the same two steps as the launch -- the
 * struct_size check and the one planning function -- and scratch counts as available exactly as there: `workspace` given, 16-byte
 * aligned, `workspace_bytes` large enough for the form.  Returns what the launch would return for a refused call (KEEP_EINVAL, or
 * KEEP_EUNSUP for KEEP_MMA_X1 | KEEP_ATTN_X1) with the same message; `out` is zeroed then.
 *
 *   waves / dvt / nslices   32-query waves per block (1 or 4), 32-column tiles of one block's dv slice (1 / 2 / 4), dv slices per head
 *   masked                  the bf16-input kernel's region-mask instantiation (mode 2 with shift > 0)
 *   win_tables              the launch stages the mode-2 window tables (token -> pixel, region ids) of all keys in LDS
 *   lds_bytes               dynamic LDS of the form's last launch (0: the kernel has static LDS only)
 *   scratch_bytes           what the workspace query of keep_hip.h answers for these arguments: the scratch the library could use,
 *                           whether or not the call brings it (`kernel` names the form planned with the scratch the call does bring)
 *   kernel                  the template instantiation as a profiler prints it, every template argument spelled out; a form of two
 *                           launches names both in launch order, joined by " + " (pack + flash, scores + pv)
 *
 * Tests use it to prove that their case tables reach every instantiation; it is no part of the product path. */
typedef struct {
  int32_t waves, dvt, nslices;
  int32_t masked;
  int32_t win_tables;
  int64_t lds_bytes, scratch_bytes;
  char kernel[96];
} keep_attention_plan_out;
int32_t keep_attention_plan(const keep_attention_args* a, keep_attention_plan_out* out);

/* ---- what one keep_conv2d call of keep_hip.h would launch: HOST-only C (no device, no stream; no pointer of `a` is dereferenced, they are
 * tested for presence and alignment only, so aligned made-up addresses do).  It is the launch itself with the launches taken out: the
 * arguments go through keep_conv2d's own code -- the struct_size check, validation, the plan (what keep_conv2d_plan reports), the tensor
 * and workspace requirements of a launch, and every launch-time decision that follows from the real N, the flags, the chunk count and the
 * activations -- and each place that would launch a kernel writes that kernel's name instead.  Returns what keep_conv2d would return for
 * a refused call, with the same message; `out` is zeroed then.
 *
 *   n_kernels   kernels the call launches
 *   kernels     their template instantiations as a profiler prints them (every template argument spelled out, without the return type
 *               and the parameter list), in launch order, joined by " + ": zero_u32_kernel first when x3_out_amax is given and not
 *               zeroed, then the convolution, then what follows it (a split-K reducer, a statistics replica kernel)
 *
 * keep_conv2d_plan names a call's FORM (engine policies key on that name); this names the INSTANTIATION the launch takes for it.  Tests
 * use it to prove that their case tables reach every instantiation; it is no part of the product path. */
typedef struct {
  int32_t n_kernels;
  char kernels[508];
} keep_conv2d_launch_plan_out;
int32_t keep_conv2d_launch_plan(const keep_conv2d_args* a, keep_conv2d_launch_plan_out* out);

/* ---- GMFlow window attention without the K / V pack pass (KEEP_MMA_X3).  The projection GEMM writes k and v already split, the attention
 * kernel reads them as they are: the pack kernel's pass over both tensors (read fp32, split, gather, transpose, write) does not run, and
 * every product sees the operand bits the packed path gives it -- same results, bit for bit.
 *
 * keep_conv2d_split: the core header's convolution entry with output columns [split_c0, split_c1) written as split-fp16 halves: column c of
 * 128-column group g stores hi = (fp16)y at byte g * 512 + (c % 128) * 2 of the output row and lo = (fp16)(y - (float)hi) 256 bytes further
 * on -- the same 512 bytes per group, so strides and allocation stay those of the fp32 tensor; columns outside the range stay fp32.  For
 * the KEEP_MMA_X3 GEMM form only (1x1, stride 1, no prologue / activation / residual / aux / split-K / statistics / LayerNorm): fp32
 * output, Cout, out_ld and both bounds multiples of 128, N * Ho * Wo a multiple of 128; KEEP_EUNSUP otherwise.  keep_conv2d_split_plan is
 * the core plan query for such a call (host only).
 *
 * keep_attention_kv_split: the core header's attention entry on k / v pointers into such a tensor (per token [hi x 128 | lo x 128] fp16 in
 * the 512 bytes of the 128 floats; strides stay in fp32 elements).  The kernel gathers the window rows itself and takes V through the
 * transposed LDS read; `workspace` is not used.  KEEP_MMA_X3, fp32 in_dtype, mode 2, D = Dv = 128, H = 1, Lq a multiple of 128, Lk a
 * multiple of 32 and <= 4096, no range probes, 16-byte aligned q rows, k / v strides multiples of 128; KEEP_EUNSUP otherwise -- the caller
 * then keeps the fp32 tensor and the core entry.  keep_attention_kv_split_plan answers without a launch (host only): `kernel` names the
 * one launch, scratch_bytes is 0. */
int32_t keep_conv2d_split(const keep_conv2d_args* a, int32_t split_c0, int32_t split_c1, void* stream);
int32_t keep_conv2d_split_plan(const keep_conv2d_args* a, int32_t split_c0, int32_t split_c1, keep_conv2d_plan_out* out);
int32_t keep_attention_kv_split(const keep_attention_args* a, void* stream);
int32_t keep_attention_kv_split_plan(const keep_attention_args* a, keep_attention_plan_out* out);

/* ---- the GMFlow feed-forward block of keep_hip.h's fused x3 entry on SINGLE fp16 operands (opt-in speed form, outside the 1e-3 parity
 * tolerance):
 *
 *     out = LayerNorm( W2 . gelu( W0 . cat[src | msg] ) ; gamma, beta, eps ) + src          src, msg, out [M, C] fp32,  C = 128
 *
 * cat[src | msg] is rounded once to fp16 (the conversion of the x3 `hi` half), every GELU output once more in front of the second product;
 * one fp16 MFMA per product, fp32 accumulation; scale, GELU (exact_act != 0: erff, else the fast form), LayerNorm and + src in fp32 on the
 * unrounded src.  The argument list is the x3 entry's; the weights are hi-only twins, ONE fp16 bit pattern per weight, with the x3
 * twins' power-of-two scales (w0_acc_scale / w2_acc_scale = 2^-e):
 *   w0_x1    [hidden][2C]   fp16(W0 * 2^e0), plain row-major
 *   w2p_x1   [C][hidden]    fp16(W2p * 2^e2), W2p = W2 with every group of 16 hidden units in the order [0-3, 8-11, 4-7, 12-15]
 * -- the numbers of the x3 twins' hi halves.  KEEP_EINVAL before anything is launched, the message naming the function: a null pointer,
 * M <= 0, C != 128, hidden <= 0 or hidden % 32 != 0, a pointer that is not 16-byte aligned, weight tensors of 2 GB or more.
 *
 * keep_gm_ffn_x1_plan: HOST-only C (no device, no stream): does the library have the single-fp16 form for this per-token shape?  The
 * alignment classes are `address % 16` OR-ed over the tensors of a class -- src / msg / out, the two weight twins, gamma / beta -- 0 when
 * all are 16-byte aligned.  KEEP_OK, or KEEP_EUNSUP with the reason as the thread's last error message -- the caller stays on the x3 entry; KEEP_EINVAL
 * for a non-positive C / hidden or a negative class.  M is no argument: the answer never depends on the token count. */
int32_t keep_gm_ffn_x1_plan(int32_t C, int32_t hidden, int32_t io_misalign, int32_t weight_misalign, int32_t ln_misalign);
int32_t keep_gm_ffn_x1(const float* src, const float* msg, const void* w0_x1, float w0_acc_scale, const void* w2p_x1, float w2_acc_scale,
                       const float* ln_gamma, const float* ln_beta, float ln_eps, float* out, int64_t M, int32_t C, int32_t hidden,
                       int32_t exact_act, void* stream);

/* ---- the scene-cut signature of a frame (modules/scene_cuts.py: frame_signature_host is the same arithmetic on the host): a 4 x 4 grid of
 * 16-bin luma histograms, integers throughout.  Per pixel (x, y) of frame n:
 *
 *     Y = (29 * B + 150 * G + 77 * R + 128) >> 8      (the weights sum to 256: Y <= 255)
 *     sig[n][(((y * 4) / H) * 4 + (x * 4) / W) * 16 + (Y >> 4)] += 1
 *
 * so the 256 counters of a frame sum to H * W.  keep_frame_signature_u8: `frames` [N,H,W,3] uint8 BGR and `sig` [N,256] int32 are
 * contiguous DEVICE memory; `frames` needs NO alignment (a view into a larger buffer does).  `sig` is OVERWRITTEN: its zero-fill is
 * queued on `stream` in front of the counting kernel, which adds one total per (block, counter) with vector global atomics on integers.
 * A frame's counters therefore depend neither on N, on the frames beside it, on the launch geometry nor on the run.  KEEP_EINVAL, before
 * anything is launched: a null pointer; N, H or W <= 0; H or W >= 32768. */
int32_t keep_frame_signature_u8(const uint8_t* frames /*device [N,H,W,3] BGR*/, int32_t N, int32_t H, int32_t W,
                                int32_t* sig /*device [N,256]*/, void* stream);

/* ---- the paste-back composite of one face with a weight (track lifetimes: a face fades in and out at the ends of its lifetime).  The
 * arguments, the two mask forms (mask_border >= 0: the blurred parse mask in face space; mask_border < 0: a soft mask in frame space) and
 * every operation are those of the core header's keep_paste_face -- one kernel serves both entries -- with one float32 product added:
 *
 *     soft = soft * opacity            (directly after the soft mask value is formed, rounded on its own)
 *     frame = soft * face + (1 - soft) * frame
 *
 * opacity 1.0f is the core entry bit for bit, 0.0f leaves `frame` bit-identical.  KEEP_EINVAL, before anything is launched: the core
 * entry's refusals, and an opacity outside [0, 1] or NaN. */
int32_t keep_paste_face_w(float* frame /*device [H,W,3]*/, int32_t H, int32_t W, const uint8_t* face /*device [fh,fw,3]*/,
                          const float* mask /*device*/, int32_t fh, int32_t fw, const double* dst_to_src /*host [6]*/, int32_t x0, int32_t y0,
                          int32_t x1, int32_t y1, int32_t mask_border, float opacity, void* stream);

/* ---- the alias-free paste-back composite of one face (opt-in, engine/paste.py: GpuPaster.paste(aa=True)).  keep_paste_face takes ONE
 * bilinear tap per frame pixel, a filter one crop pixel wide; a face that is shrunk on its way back (crop -> frame scale r < 1) aliases.
 * Here every frame pixel of the box is the mean of n x n sub-samples: `dst_to_src` is the destination -> source map of the n-times finer
 * frame grid (the inverse of engine/paste.py's ss_affine(M, n)), the box and the frame stay in frame pixels, and sub-sample (i, j) of
 * frame pixel (x, y) is keep_paste_face's coordinate and tap arithmetic -- 1/1024 rounding, 1/32 truncation, +-32768 clamp, taps outside
 * the crop read 0, the mask's border zeroing and / 255 -- at the integer position (n x + i, n y + j) with that map:
 *
 *     v_k[c] = (taps . 15-bit weights + 2^14) >> 15                       0 .. 255
 *     q_k    = rint(s_k * 65536), half to even, int32                     s_k: keep_paste_face's float soft mask value (mask_border >= 0)
 *     S_c = sum_k v_k[c],  Q = sum_k q_k                                  int32: the order is free
 *     face_c = float(S_c) * (1 / n^2),  soft = float(Q) * (1 / (65536 n^2))
 *     soft = soft * opacity;  frame = soft * face_c + (1 - soft) * frame  the separately rounded float32 operations of keep_paste_face_w
 *
 * Bounds: a blurred 0/255 mask divided by 255 reaches 1.0000006, so q_k <= 65537 and Q < 2^23; S_c <= 64 * 255 = 16320: both
 * conversions and both power-of-two scalings are exact.  mask_border < 0 (the frame-space soft mask): soft = mask[y, x] as in the core
 * entry, only the face is supersampled.  Not a restatement of the reference (which aliases); below r = 1/8 the sub-samples of n = 8 lie
 * more than one crop pixel apart and residual aliasing stays.  KEEP_EINVAL, before anything is launched: everything keep_paste_face_w
 * refuses, and n outside {2, 4, 8}. */
int32_t keep_paste_face_aa(float* frame /*device [H,W,3]*/, int32_t H, int32_t W, const uint8_t* face /*device [fh,fw,3]*/,
                           const float* mask /*device*/, int32_t fh, int32_t fw, const double* dst_to_src /*host [6], of the n-times grid*/,
                           int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t mask_border, int32_t n, float opacity, void* stream);

/* ---- tone match of restored faces (engine/tone.py): the restored face keeps its high band and takes the low band of the crop it was made
 * from,  out = rst + lowpass(src - rst),  a separable Gaussian in integers throughout.  Per channel, indices clamped at the borders
 * (replicate), taps t[-R .. R]:
 *
 *     d  = src - rst                                  [-255, 255]
 *     hh = sum_k t[k] * d[y, clamp(x + k, 0, w - 1)]  int32
 *     h4 = (hh + 128) >> 8                            (arithmetic shift = floor) |h4| <= 4080: int16, 4 fractional bits
 *     v  = sum_k t[k] * h4[clamp(y + k, 0, h - 1), x] int32
 *     out = clamp(rst + ((v + 32768) >> 16), 0, 255)
 *
 * No float and no atomic: the result depends neither on the summation order, the launch geometry nor F.  src == rst gives out == rst;
 * src == rst + c without saturation gives out == src.
 *
 * keep_tone_match_u8: `src`, `rst`, `out` [F,h,w,3] uint8 and `scratch` (F*h*w*3 int16, contents afterwards unspecified) are contiguous
 * DEVICE memory of any alignment; `taps` [2R+1] is a HOST array, read and validated before the call returns -- the int32 bounds above rest
 * on that check -- and travels in the kernel arguments: no allocation, no copy.  Two kernels per launch group on `stream`, F split where a
 * grid extent would pass 2^31.  KEEP_EINVAL, before anything is launched: a null pointer; F, h or w <= 0; h or w >= 32768; R outside
 * 1 .. 128; a negative tap; taps that do not sum to 4096; `out` or `scratch` overlapping `src`, `rst` or each other as byte ranges (a block
 * reads its neighbours' pixels through the halo: in place is a race). */
int32_t keep_tone_match_u8(const uint8_t* src, const uint8_t* rst, uint8_t* out, int16_t* scratch, int32_t F, int32_t h, int32_t w,
                           const int16_t* taps /*host [2R+1]*/, int32_t R, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* KEEP_CV_HIP_H */
