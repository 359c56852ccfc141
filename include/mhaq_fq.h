/*
 * mhaq_fq.h -- C ABI of the MI355X-native fake-quantization path for MHAQ.
 *
 * Drop-in boundary.  The reference has no native code:
 * its "operator seam" is the Python class `Quantizer` and the autograd
 * Functions `QN*` in
 *     /root/reference/src/quantization/gdnsq/gdnsq.py:11-241
 * driven by the layer wrappers
 *     /root/reference/src/quantization/gdnsq/layers/gdnsq_act.py:39-55
 *     /root/reference/src/quantization/gdnsq/layers/gdnsq_conv2d.py:71-100
 *     /root/reference/src/quantization/gdnsq/layers/gdnsq_linear.py:61-78
 * Each entry point below names the reference lines whose eager op chain it
 * replaces.  INTEGRATION.md shows the ctypes / autograd.Function binding a
 * maintainer of the reference would add.
 *
 * Conventions (all entry points):
 *   - plain C, no torch / C++ types; every pointer is a DEVICE pointer to
 *     contiguous fp32 unless stated otherwise; sizes are element counts.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - Devices: a call launches on `stream` and holds no device state of its own.  As with any HIP library that takes a
 *     stream, the calling thread's CURRENT device must be the device `stream` and every pointer belong to (with the NULL
 *     stream: the current device's default stream).  The host side above this ABI provides that for tensors on any device:
 *     the compiled autograd nodes and the ctypes ops switch to their input's device for the duration of a call
 *     (mhaq_amd/csrc/torch_binding.cpp MHAQ_ON_DEVICE_OF, mhaq_amd/ops.py _on_device), as torch's own ops do.
 *     (Those host-side switches have run with ONE visible device only -- the training boxes are one process per GPU --;
 *     tests/test_gpu_two_devices.py exercises them and is skipped until a process sees two devices: a model on another
 *     device than the current one is untested on hardware.)
 *   - stream-ordered and asynchronous: no host synchronisation, no allocation,
 *     no state kept between calls (a launch's status travels to the return statement in a thread-local word; one
 *     device attribute is memoised per device) -> re-entrant, thread-safe, hipGraph-capture-safe.  `seed` / `offset` of the random
 *     sign stream are host arguments, which a captured launch freezes; every backward entry point therefore
 *     also takes `offset_dev`, a nullable DEVICE pointer to one uint64 that the kernel adds to `offset`
 *     (effective offset = offset + *offset_dev, mod 2^64).  A captured training step keeps that word in
 *     memory and advances it once per replay (one 8-byte add), so replay k of a launch captured with host
 *     offset c draws the stream (seed, c + k * stride): fresh signs per step at 0 extra bytes per element.
 *     NULL = host offset only (eager callers).
 *   - the caller owns every buffer, including `workspace` (query the size
 *     with the matching *_workspace_bytes(); contents need no initialisation).
 *   - scalar quantizer parameters (scale, zero point, clamp bounds) are
 *     DEVICE pointers: they are live autograd tensors in the caller and must
 *     not be read back to the host.
 *   - return value: 0 = ok; >0 = hipError_t of the failed launch;
 *     <0 = argument error (MHAQ_FQ_E*).  Nothing throws.
 *
 * Map to the export list sketched in SURVEY.md section 8b:
 *   mhaq_fq_act_fwd / mhaq_fq_act_bwd        -> same names (NoisyAct from its learnable parameters);
 *                                               mhaq_fq_pt_fwd / _bwd take (s, zp, lo, hi) tensors instead
 *   mhaq_fq_w_fwd / mhaq_fq_w_bwd            -> mhaq_fq_wlayer_fwd / _bwd (per-channel, from log_wght_s),
 *                                               mhaq_fq_pc_fwd / _bwd (given scales), mhaq_fq_wlayer_pt_*
 *                                               and mhaq_fq_minmax + mhaq_fq_pt_* + tie_scatter (per-tensor)
 *   mhaq_fq_w_aewgs_stats -> [3,Co], _apply  -> mhaq_fq_pc_aewgs_stats, then *_bwd with `stats` != NULL
 *   multi-tensor variants (pointer table)    -> mhaq_fq_wlayer_fwd_multi / _bwd_multi
 *
 * Arithmetic contract: fp32 throughout, IEEE-correct division, round half to
 * even, no FMA contraction -- every elementwise output (y, q, gx, wq) is
 * bit-identical to the reference's eager chain on the same inputs.  Reduced
 * gradients are accumulated in fp64 and rounded once (deterministic: fixed
 * partition + fixed-order final sum, no float atomics).
 */
#ifndef MHAQ_FQ_H
#define MHAQ_FQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHAQ_FQ_ABI_VERSION 4   /* v2: every backward entry point takes `offset_dev`; v3: sign stream layout (128 elements per Philox call);
                                  v4 (additive): mhaq_fq_pc_quantize; later additive entry points
                                  (the 16-bit activation path, *_x16) keep v4 and are discovered by symbol */

/* Estimator selector == QNMethod value (gdnsq_utils.py:9-13). */
enum { MHAQ_FQ_STE = 0, MHAQ_FQ_EWGS = 1, MHAQ_FQ_AEWGS = 2, MHAQ_FQ_LSQ = 3 };

/* Argument errors. */
enum {
  MHAQ_FQ_EINVAL = -1,     /* null pointer / negative size / unknown method */
  MHAQ_FQ_EWORKSPACE = -2, /* workspace smaller than *_workspace_bytes()     */
  MHAQ_FQ_EALIGN = -3,     /* pointer not 4-byte aligned                     */
  MHAQ_FQ_EUNSUPPORTED = -4
};

/* Flag bits written by the eval-mode integrity check (gdnsq.py:211-217). */
enum {
  MHAQ_FQ_FLAG_BELOW_MIN = 1, /* some q < floor((min_val-zp)/s) */
  MHAQ_FQ_FLAG_ABOVE_MAX = 2, /* some q > ceil((max_val-zp)/s)  */
  MHAQ_FQ_FLAG_NOT_INTEGER = 4
};

int mhaq_fq_abi_version(void);
const char* mhaq_fq_error_string(int code);

/* ------------------------------------------------------------------------
 * Random sign stream of the stochastic scale gradient (gdnsq.py:54,104,144:
 * r = randint_like(v, 2) - 0.5).  In-kernel Philox4x32-10, layout v3 (ABI v3): ONE Philox call
 * yields the signs of 128 CONSECUTIVE elements -- all 128 output bits are spent.  Element i of a
 * call with (seed, offset):
 *     c = i >> 7                                      (the Philox call)
 *     out[0..3] = Philox4x32-10(counter = {lo(c), hi(c), lo(offset), hi(offset)},
 *                               key     = {lo(seed), hi(seed)})
 *     j = i & 127;   r = ((out[j >> 5] >> (j & 31)) & 1) ? +0.5 : -0.5
 * A pure function of (seed, offset, i): independent of the launch geometry.  (Layouts v1 / v2 drew
 * one call per lane and used 8 of its 128 bits; a workgroup now computes the calls its elements need
 * once, into LDS, and every lane shifts its bits out of them.)  mhaq_fq_fill_r materialises the
 * stream as int8 signs (+1/-1) so a checker can replay a backward with an explicit `r`;
 * tests/philox_ref.py restates the layout in numpy and holds mhaq_fq_fill_r to it.
 * Every backward entry point takes `r_sign`: non-NULL = read signs from
 * memory (int8, 1 B/elem extra: a positive value is +0.5, zero or negative is -0.5, so both the
 * +-1 coding of mhaq_fq_fill_r and a 0/1 coding such as torch.randint(0, 2) work), NULL = generate in-kernel.
 * ---------------------------------------------------------------------- */
int mhaq_fq_fill_r(int8_t* r_sign, int64_t n, uint64_t seed, uint64_t offset, void* stream);

/* ------------------------------------------------------------------------
 * Per-tensor fake-quant (one scale / zero point / clamp range for the whole
 * tensor): the activation quantizer NoisyAct (gdnsq_act.py:39-55) and the
 * elementwise half of a PER_TENSOR weight quantizer.
 *
 * Forward: replaces Quantizer.quantize + dequantize (gdnsq.py:189-229):
 *   v0 = clamp(x, *lo, *hi); v = (v0 - *zp) / *s; q = v + (rne(v) - v);
 *   y = q * *s + *zp
 * y may alias x.  Optional outputs (NULL to skip):
 *   q_out     [n]  the rounding indices (integer-valued fp32)
 *   qstats    [2]  {min q, max q} for NoisyAct.bw = log2(max-min+1)
 *                  (gdnsq_act.py:51-54); needs workspace
 *   flags     [1]  int32 OR of MHAQ_FQ_FLAG_* (eval asserts, no host sync)
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_pt_fwd_workspace_bytes(int64_t n);
int mhaq_fq_pt_fwd(const float* x, float* y, int64_t n,
                   const float* s, const float* zp, const float* lo, const float* hi,
                   float* q_out, float* qstats, int32_t* flags,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Backward of the same chain given g = dL/dy; replaces the autograd graph of
 * gdnsq.py:197-208,229 + QN*.backward (gdnsq.py:35-57,63-84,90-107):
 *   gq = g * s; gv = gq + estimator(gq, e); g1 = gv / s;
 *   gx = g1 * [lo <= x <= hi]                                (gx may alias g)
 *   grads[0] = dL/ds  = sum g*q - sum gv*(v/s) + noise_term
 *   grads[1] = dL/dzp = sum g - sum g1
 *   grads[2] = dL/dlo = sum g1*[x < lo]     (0 if lo > hi)
 *   grads[3] = dL/dhi = sum g1*[x > hi]     (all of sum g1 if lo > hi)
 *   grads[4] = number of elements with x == zp (tie count for amin backward;
 *              only when count_ties != 0)
 * count_ties != 0 is the weight-quantizer mode, whose bounds never clip (lo = -inf; hi = +inf or the
 * tensor's own maximum): dL/dhi is identically 0 there and grads[3] carries the number of elements with
 * x == hi instead (the amax tie count mhaq_fq_wlayer_ptl_bwd needs; 0 for hi = +inf).
 * noise_term = 3^-1/2 sum gq*r (STE, EWGS, AEWGS) or sum gq*(q-v) (LSQ).
 * method: MHAQ_FQ_STE, MHAQ_FQ_LSQ, MHAQ_FQ_EWGS (as intended; the reference
 * raises at gdnsq.py:102), or MHAQ_FQ_AEWGS with `col_stats` [3][period]
 * (mean sign(gq)*e, mean e^2, mean e per position i % period: the reference's
 * reduce_to_shape quirk for a [1]-shaped scale, gdnsq.py:150-152).
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_pt_bwd_workspace_bytes(int64_t n);
int mhaq_fq_pt_bwd(const float* x, const float* g, float* gx, int64_t n,
                   const float* s, const float* zp, const float* lo, const float* hi,
                   int method, const float* col_stats, int64_t period,
                   const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                   int count_ties /* 0: grads[4] is left 0 (activations) */,
                   float* grads /* [5] */,
                   void* workspace, size_t workspace_bytes, void* stream);

/* The two launches of mhaq_fq_pt_bwd, separately (bench.py times the streaming kernel on its
 * own; a multi-tensor caller can batch the finalizes): *_partials runs the streaming kernel and
 * leaves `*nparts_out` partial rows in `workspace`; *_finalize reduces them to grads[5]. */
int mhaq_fq_pt_bwd_partials(const float* x, const float* g, float* gx, int64_t n,
                            const float* s, const float* zp, const float* lo, const float* hi,
                            int method, const float* col_stats, int64_t period,
                            const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, int count_ties,
                            void* workspace, size_t workspace_bytes, int32_t* nparts_out, void* stream);
int mhaq_fq_pt_bwd_finalize(const void* workspace, int32_t nparts, float* grads /* [5] */, void* stream);

/* ------------------------------------------------------------------------
 * NoisyAct from its LEARNABLE parameters (gdnsq_act.py:39-55): the scalar chain
 * s = exp2(log_act_s), qr = exp2(log_act_q), zp = min_val = act_b, max_val = act_b + qr - s and
 * its backward are folded into the same two launches (the eager reference spends ~12 extra
 * launches per quantizer per step on them).
 *   act_fwd: as mhaq_fq_pt_fwd; writes params_out[5] = {s, zp, lo, hi, qr} for the backward and
 *            for side consumers of Quantizer.scale / zero_point / min_val / max_val.
 *   act_bwd: as mhaq_fq_pt_bwd with `params` from the forward; grads[3] =
 *            {dL/dlog_act_s, dL/dlog_act_q, dL/dact_b}.  method: STE, LSQ or EWGS.
 * ---------------------------------------------------------------------- */
int mhaq_fq_act_fwd(const float* x, float* y, int64_t n,
                    const float* log_act_s, const float* log_act_q, const float* act_b,
                    float* params_out /* [5] */, float* qstats, int32_t* flags,
                    void* workspace, size_t workspace_bytes, void* stream);
size_t mhaq_fq_act_bwd_workspace_bytes(int64_t n);
int mhaq_fq_act_bwd(const float* x, const float* g, float* gx, int64_t n, const float* params /* [5] */,
                    int method, const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                    float* grads /* [3] */, void* workspace, size_t workspace_bytes, void* stream);

/* The two launches of mhaq_fq_act_bwd, separately, so that ONE finalize serves every activation quantizer of
 * a backward pass (the scalar gradients are only needed by the optimizer): *_partials runs the streaming
 * kernel, leaves `*nparts_out` partial rows in `workspace` and {s, qr} behind them; *_finalize_multi reduces
 * the workspaces of `nquant` such calls (device-resident table; a caller that keeps its workspaces alive
 * across steps uploads the table once) into grads_out[nquant][3] = {dL/dlog_act_s, dL/dlog_act_q, dL/dact_b}
 * per quantizer -- bit-identical to the per-quantizer finalize of mhaq_fq_act_bwd. */
typedef struct {
  const float* partials; /* the `workspace` of one mhaq_fq_act_bwd_partials call */
  int64_t nparts;        /* its *nparts_out */
} mhaq_act_finalize_desc;
int mhaq_fq_act_bwd_partials(const float* x, const float* g, float* gx, int64_t n, const float* params /* [5] */,
                             int method, const int8_t* r_sign, uint64_t seed, uint64_t offset,
                             const uint64_t* offset_dev, void* workspace, size_t workspace_bytes,
                             int32_t* nparts_out, void* stream);
int mhaq_fq_act_bwd_finalize_multi(const mhaq_act_finalize_desc* descs_device, int nquant,
                                   float* grads_out /* [nquant][3] */, void* stream);

/* ------------------------------------------------------------------------
 * 16-bit activations (mixed-precision training under torch.autocast: the convolution in front of a NoisyAct hands it a
 * bf16 / fp16 tensor).  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by
 * symbol.  They mirror mhaq_fq_act_fwd / _bwd / _bwd_partials with untyped data pointers and an element type:
 *   x, y, g, gx   16-bit (dtype), contiguous in memory order, at least 2-byte aligned (else MHAQ_FQ_EALIGN);
 *                 16-byte aligned pointers take the 8-elements-per-lane kernels, others an element kernel
 *   params, grads, qstats, log_act_s / log_act_q / act_b   fp32, as in the fp32 entry points
 *   dtype         MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16 (anything else: MHAQ_FQ_EINVAL)
 * Arithmetic: every element is converted up exactly and runs the fp32 chain above; y and gx are rounded to nearest-even
 * once.  y == RNE(y of mhaq_fq_act_fwd on the upcast x), gx == RNE(gx of mhaq_fq_act_bwd on the upcast x and g),
 * element i draws the same random sign as the fp32 backward at the same (seed, offset, offset_dev), and the parameter
 * gradients are the fp32 ones.
 * Workspace rule: a call needs no more than the matching fp32 query returns -- mhaq_fq_pt_fwd_workspace_bytes(n) for
 * the eval form of _fwd_x16 (qstats / flags non-NULL), mhaq_fq_act_bwd_workspace_bytes(n) for the backward; the 16-bit
 * launch geometry never leaves more partial rows than the fp32 one (MHAQ_FQ_EWORKSPACE otherwise).  The partial rows
 * of _bwd_partials_x16 have the layout of mhaq_fq_act_bwd_partials: mhaq_fq_act_bwd_finalize_multi reduces 16-bit and
 * fp32 quantizers in the same launch.
 * ---------------------------------------------------------------------- */
enum { MHAQ_FQ_DT_F32 = 0 /* only where an entry point says so */, MHAQ_FQ_DT_BF16 = 1, MHAQ_FQ_DT_F16 = 2 };
int mhaq_fq_act_fwd_x16(const void* x, void* y, int64_t n, int dtype,
                        const float* log_act_s, const float* log_act_q, const float* act_b,
                        float* params_out /* [5] */, float* qstats, int32_t* flags,
                        void* workspace, size_t workspace_bytes, void* stream);
int mhaq_fq_act_bwd_x16(const void* x, const void* g, void* gx, int64_t n, int dtype, const float* params /* [5] */,
                        int method, const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                        float* grads /* [3] */, void* workspace, size_t workspace_bytes, void* stream);
int mhaq_fq_act_bwd_partials_x16(const void* x, const void* g, void* gx, int64_t n, int dtype,
                                 const float* params /* [5] */, int method, const int8_t* r_sign, uint64_t seed,
                                 uint64_t offset, const uint64_t* offset_dev, void* workspace, size_t workspace_bytes,
                                 int32_t* nparts_out, void* stream);

/* ------------------------------------------------------------------------
 * NoisyAct behind a ReLU (and a residual add), in the quantizer's own launches.  Additive to ABI v4 --
 * MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.  fp32; STE, LSQ or EWGS.
 *   relu_fwd:  a = relu(z + addend) (addend nullable: a = relu(z)), y = fake_quant(a) as mhaq_fq_act_fwd computes it,
 *              params_out[5] as there; a is written to a_out when that is non-NULL.  relu = torch.relu: NaN passes.
 *              z, addend, y, a_out must not overlap.
 *   relu_bwd:  z = the ReLU's input OR its output (a = relu(z) either way), g_y = dL/dy, g_a = the gradient reaching a
 *              from its other consumers (nullable):  gx = (z <= 0) ? 0 : (gx of mhaq_fq_act_bwd(a, g_y) + g_a).
 *              The partial rows (count, layout, values, {s, qr} behind them), the workspace rule, the random signs at
 *              (seed, offset, offset_dev) and grads[3] are those of mhaq_fq_act_bwd_partials / mhaq_fq_act_bwd on
 *              (a, g_y): mhaq_fq_act_bwd_finalize_multi serves both kinds of launch.
 * Pointers at least 4-byte aligned (MHAQ_FQ_EALIGN); 16-byte aligned ones take the float4 kernels.
 * ---------------------------------------------------------------------- */
int mhaq_fq_act_relu_fwd(const float* z, const float* addend, float* y, float* a_out, int64_t n,
                         const float* log_act_s, const float* log_act_q, const float* act_b,
                         float* params_out /* [5] */, void* stream);
int mhaq_fq_act_relu_bwd(const float* z, const float* g_y, const float* g_a, float* gx, int64_t n,
                         const float* params /* [5] */, int method, uint64_t seed, uint64_t offset,
                         const uint64_t* offset_dev, float* grads /* [3] */, void* workspace, size_t workspace_bytes,
                         void* stream);
int mhaq_fq_act_relu_bwd_partials(const float* z, const float* g_y, const float* g_a, float* gx, int64_t n,
                                  const float* params /* [5] */, int method, uint64_t seed, uint64_t offset,
                                  const uint64_t* offset_dev, void* workspace, size_t workspace_bytes,
                                  int32_t* nparts_out, void* stream);

/* ------------------------------------------------------------------------
 * The same on 16-bit tensors (a NoisyAct behind a ReLU under torch.autocast).  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION
 * stays 4; a caller discovers these entry points by symbol.  z, addend, y, a_out, g_y, g_a, gx are 16-bit (dtype =
 * MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16, else MHAQ_FQ_EINVAL), at least 2-byte aligned (MHAQ_FQ_EALIGN); 16-byte aligned
 * ones with n >= 8 take the 8-elements-per-lane kernels, others an element kernel.  params, grads and the quantizer's
 * parameters are fp32.  STE, LSQ or EWGS.
 * Arithmetic: the BITS of the separate 16-bit launches -- the framework's 16-bit add, relu, threshold_backward and
 * gradient accumulation around the 16-bit entry points above -- not a single-rounding variant of them.  With up = the exact
 * conversion to fp32 and R = round to nearest-even to dtype (NaN stays NaN):
 *   relu_fwd:  t = addend ? R(up(z) + up(addend)) : z;   a = relu(t) (NaN passes), written to a_out when non-NULL;
 *              y = R(fake_quant(up(a))), what the 16-bit forward above gives on a.
 *   relu_bwd:  a = relu(up(z)) (z = the ReLU's input or its output);   gq = R(gx of the fp32 backward on (a, up(g_y)));
 *              gs = g_a ? R(up(gq) + up(g_a)) : gq;   gx = (up(z) <= 0) ? +0 : gs   (a NaN z passes the gradient).
 *              gs is rounded TWICE on purpose: unfused, the quantizer writes a 16-bit gq and the framework adds the other
 *              consumer's 16-bit gradient with a 16-bit add.  R(unrounded gq + g_a) would be nearer the exact sum, and
 *              another training run than the one the separate launches give.
 * The partial rows (count, layout, values, {s, qr} behind them), the random signs at (seed, offset, offset_dev) and
 * grads[3] are those of the 16-bit backward above on (a, g_y), byte for byte: the parameter sums take the fp32 values of
 * every element, masked or not.  The workspace is the fp32 query's for n, and the finalize of several quantizers serves
 * fused and plain, 16-bit and fp32 launches together.  Stream-ordered, no host synchronisation, capture-safe.
 * ---------------------------------------------------------------------- */
int mhaq_fq_act_relu_fwd_x16(const void* z, const void* addend, void* y, void* a_out, int64_t n, int dtype,
                             const float* log_act_s, const float* log_act_q, const float* act_b,
                             float* params_out /* [5] */, void* stream);
int mhaq_fq_act_relu_bwd_x16(const void* z, const void* g_y, const void* g_a, void* gx, int64_t n, int dtype,
                             const float* params /* [5] */, int method, uint64_t seed, uint64_t offset,
                             const uint64_t* offset_dev, float* grads /* [3] */, void* workspace,
                             size_t workspace_bytes, void* stream);
int mhaq_fq_act_relu_bwd_partials_x16(const void* z, const void* g_y, const void* g_a, void* gx, int64_t n, int dtype,
                                      const float* params /* [5] */, int method, uint64_t seed, uint64_t offset,
                                      const uint64_t* offset_dev, void* workspace, size_t workspace_bytes,
                                      int32_t* nparts_out, void* stream);

/* ------------------------------------------------------------------------
 * Backward of training-mode BatchNorm (torch.nn.BatchNorm2d on a channels_last tensor) from the statistics its forward
 * saved.  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.
 *   x, dy, dx       dense fp32 NHWC seen as [m = N*H*W][c]; c % 4 == 0 and c <= 2^22 (else MHAQ_FQ_EUNSUPPORTED);
 *                   x, dy, dx and `workspace` 16-byte aligned (else MHAQ_FQ_EALIGN)
 *   mean, invstd    [c], the batch statistics of the forward (invstd = (var + eps)^-1/2)
 *   weight          [c], NULL = 1
 *   dbias   = sum_rows dy                                dweight = invstd * sum_rows dy * (x - mean)
 *   dx      = (weight * invstd) * ((dy - dbias / m) - ((x - mean) * invstd) * (dweight / m))
 * Any of dx, dweight, dbias may be NULL (dx == NULL skips its launch).  Three launches: partial sums (x and dy read once,
 * fp32 per lane, one partial row per block in `workspace`), a fixed-order fp64 final sum, the dx stream -- deterministic,
 * no float atomics.
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_bn_bwd_workspace_bytes(int64_t m, int64_t c);
int mhaq_fq_bn_bwd(const float* x, const float* dy, const float* mean, const float* invstd, const float* weight,
                   float* dx, float* dweight, float* dbias, int64_t m, int64_t c,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Forward of training-mode BatchNorm on the same tensors (fp32).  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION stays 4; a
 * caller discovers these entry points by symbol.
 *   x, y            dense fp32 NHWC seen as [m][c]; m >= 2 (the unbiased variance), c % 4 == 0 and c <= 2^22 (else
 *                   MHAQ_FQ_EUNSUPPORTED); x, y and `workspace` 16-byte aligned (else MHAQ_FQ_EALIGN).  y == NULL skips the
 *                   third launch (statistics only).
 *   weight, bias    [c]; NULL = 1 and NULL = 0
 *   save_mean, save_invstd      [c], required: what mhaq_fq_bn_bwd reads
 *   running_mean, running_var   [c], both given or both NULL (one of them alone: MHAQ_FQ_EINVAL); NULL skips the update
 * Argument errors are returned before any launch, with mhaq_fq_bn_bwd's codes in its order: required pointers and positive
 * sizes (MHAQ_FQ_EINVAL), width and range (MHAQ_FQ_EUNSUPPORTED), the workspace (MHAQ_FQ_EWORKSPACE), the alignment.
 * Arithmetic: with k = x[row 0][.] as a per-channel shift, S1 = sum (x - k) and S2 = sum (x - k)^2 are fixed-order fp64 sums
 * of exact fp64 terms (x read once); in fp64, each result rounded to fp32 ONCE:
 *   mean = k + S1 / m        var = max(S2 / m - (S1 / m)^2, 0)  (biased)        invstd = (var + eps)^-1/2
 *   running_mean = (1 - factor) * running_mean + factor * mean
 *   running_var  = (1 - factor) * running_var  + factor * var * m / (m - 1)
 * and, in fp32, in this order, without contraction, with a = weight * save_invstd (an fp32 product):
 *   y = (x - save_mean) * a + bias
 * A constant channel gives mean = the constant, var = 0 and y = bias exactly; a channel that holds a NaN or an infinity is NaN
 * in every element of y and in its statistics.  Three launches, deterministic (y, the statistics and every byte of the
 * workspace), no float atomics.  Stream-ordered, capture-safe, stateless.
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_bn_fwd_workspace_bytes(int64_t m, int64_t c);
int mhaq_fq_bn_fwd(const float* x, const float* weight, const float* bias, float* y,
                   float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                   double factor, double eps, int64_t m, int64_t c,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The forward on 16-bit tensors (the BatchNorm behind a convolution under torch.autocast).  Additive to ABI v4 --
 * MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.
 *   x, y            dense NHWC seen as [m][c], of the type named by `dtype` (MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16, anything else:
 *                   MHAQ_FQ_EINVAL); m >= 2, c % 8 == 0 and c <= 2^22 (else MHAQ_FQ_EUNSUPPORTED); x, y and `workspace`
 *                   16-byte aligned (else MHAQ_FQ_EALIGN).  y == NULL skips the third launch.
 *   weight, bias, save_mean, save_invstd, running_mean, running_var and everything in `workspace`: fp32 / fp64, exactly as
 *                   in mhaq_fq_bn_fwd (weight, bias NULL = 1, 0; the running statistics both given or both NULL).
 * Argument errors are returned before any launch, with mhaq_fq_bn_fwd's codes in its order; the dtype is checked behind the
 * required pointers and positive sizes and before width and range, as in mhaq_fq_bn_bwd_x16.
 * Arithmetic: the contract of mhaq_fq_bn_fwd on the exactly upcast input.  With k = up(x[row 0][.]), S1 = sum (up(x) - k) and
 * S2 = sum (up(x) - k)^2 are fixed-order fp64 sums of exact fp64 terms; mean, invstd and the running statistics are formed in
 * fp64 as above and each rounded to fp32 ONCE; and, with a = weight * save_invstd (an fp32 product),
 *   y = R16((up(x) - save_mean) * a + bias)
 * is evaluated in fp32 in this order, without contraction, and rounded to nearest-even ONCE (a plain conversion: NaN stays
 * NaN, an fp16 overflow gives +-inf).  The clamp of var at 0 is a select, so a channel that holds a NaN or an infinity is NaN
 * in every element of y and in its statistics; a constant channel gives mean = the constant, var = 0 and y = R16(bias) bit
 * for bit.  The partial-row geometry differs from mhaq_fq_bn_fwd's (a lane owns 8 channels): size the workspace with
 * mhaq_fq_bn_fwd_x16_workspace_bytes (0 for an unsupported shape).  Three launches, deterministic (y, the statistics and
 * every byte of the workspace), no float atomics.  Stream-ordered, capture-safe, stateless.
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_bn_fwd_x16_workspace_bytes(int64_t m, int64_t c);
int mhaq_fq_bn_fwd_x16(const void* x, const float* weight, const float* bias, void* y,
                       float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                       double factor, double eps, int64_t m, int64_t c, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The backward on 16-bit tensors (the BatchNorm behind a convolution under torch.autocast).  Additive to ABI v4 --
 * MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.
 *   x, dy, dx       dense NHWC seen as [m][c], of the type named by `dtype` (MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16, anything else:
 *                   MHAQ_FQ_EINVAL); c % 8 == 0 and c <= 2^22 (else MHAQ_FQ_EUNSUPPORTED); x, dy, dx and `workspace`
 *                   16-byte aligned (else MHAQ_FQ_EALIGN)
 *   mean, invstd, weight, dweight, dbias and everything in `workspace`: fp32 / fp64, as above; weight and each of the
 *                   three outputs may be NULL.  Argument checks, their codes and their order are mhaq_fq_bn_bwd's, all
 *                   before any launch.
 * Arithmetic: every element is converted UP exactly and takes the arithmetic of mhaq_fq_bn_bwd unchanged -- up(x) - mean
 * and its product with up(dy) in fp64, fixed-order fp64 sums, dweight and dbias rounded once from them --, and
 *   dx = R16((weight * invstd) * ((up(dy) - dbias / m) - ((up(x) - mean) * invstd) * (dweight / m)))
 * is evaluated in fp32 in this order, without contraction, and rounded to nearest-even ONCE (a plain conversion: NaN stays
 * NaN, an fp16 overflow gives +-inf).  The partial-row geometry differs from mhaq_fq_bn_bwd's (a lane owns 8 channels):
 * size the workspace with mhaq_fq_bn_bwd_x16_workspace_bytes.  Stream-ordered, capture-safe, stateless.
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_bn_bwd_x16_workspace_bytes(int64_t m, int64_t c);
int mhaq_fq_bn_bwd_x16(const void* x, const void* dy, const float* mean, const float* invstd, const float* weight,
                       void* dx, float* dweight, float* dbias, int64_t m, int64_t c, int dtype,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The ResNet stem's max pool behind a training-mode BatchNorm: max_pool2d(kernel 3, stride 2, padding 1, dilation 1,
 * ceil_mode = false) of a dense fp32 NHWC tensor [n, h, w, c], oh = (h - 1) / 2 + 1 and ow likewise.  Additive to ABI v4.
 *   c % 4 == 0, c <= 2^22 and n * h * w < 2^31 (else MHAQ_FQ_EUNSUPPORTED); t, p, x, g, dx and `workspace` 16-byte
 *   aligned, `code` 4-byte aligned (else MHAQ_FQ_EALIGN); errors are returned before any launch.
 *
 * mhaq_fq_maxpool3s2_fwd: p[n, oh, ow, c] = the window maxima of t, code[n, oh, ow, c] (one byte each) = kh * 3 + kw of the
 * chosen element.  The selection is that of torch's channels_last kernel: the in-range positions in kh, then kw order,
 * starting at -inf, replaced on  val > max || isnan(val).  A window in which nothing replaces the start (all -inf) has
 * torch's index 0, element (0, 0) of the plane: code 4 in the window (0, 0), which contains it, and code 9 ("none chosen",
 * matched by no input element: torch's backward sends that window's gradient nowhere either) in every other window.
 *
 * mhaq_fq_bn_pool_bwd: mhaq_fq_bn_bwd on x[n, h, w, c] whose dy is the pool's backward of the pooled gradient
 * g[n, oh, ow, c], computed on the fly and never stored, with the values of torch's channels_last max_pool2d backward, bit
 * for bit: where ONE window covers (ih, iw), dy[n, ih, iw, .] is its g if its code names (ih, iw) and 0.0f if not; where
 * two or four do, dy = 0.0f plus g of every covering window whose code names (ih, iw), added in ascending oh, then ascending
 * ow.  Same partition, sums and workspace layout as mhaq_fq_bn_bwd(m = n * h * w): dx, dweight, dbias and the partial rows
 * are the bits that call gives on the materialized dy.
 * ---------------------------------------------------------------------- */
int mhaq_fq_maxpool3s2_fwd(const float* t, float* p, uint8_t* code, int64_t n, int64_t h, int64_t w, int64_t c,
                           void* stream);
size_t mhaq_fq_bn_pool_bwd_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t c);
int mhaq_fq_bn_pool_bwd(const float* x, const float* g, const uint8_t* code, const float* mean, const float* invstd,
                        const float* weight, float* dx, float* dweight, float* dbias, int64_t n, int64_t h, int64_t w,
                        int64_t c, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The stem's max pool and the gathering BatchNorm backward on 16-bit tensors (the stem under torch.autocast).  Additive to
 * ABI v4 -- MHAQ_FQ_ABI_VERSION stays 4.  t, p, x, g and dx are dense NHWC tensors of the type named by `dtype`
 * (MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16, anything else: MHAQ_FQ_EINVAL); c % 8 == 0, c <= 2^22 and n * h * w < 2^31 (else
 * MHAQ_FQ_EUNSUPPORTED); t, p, x, g, dx and `workspace` 16-byte aligned, `code` 8-byte aligned (else MHAQ_FQ_EALIGN).  mean,
 * invstd, weight, dweight, dbias and everything in `workspace` are fp32 / fp64; weight and each of the three outputs may be
 * NULL.  Argument checks, their codes and their order are those of mhaq_fq_bn_pool_bwd (the dtype check follows the NULL
 * checks), all before any launch.  Stream-ordered, capture-safe, stateless.
 *
 * mhaq_fq_maxpool3s2_fwd_x16: p and code as mhaq_fq_maxpool3s2_fwd gives them -- the same selection, compared on the exactly
 * upcast values, the same code 4 / code 9 rule -- and p holds the chosen element's ORIGINAL 16 bits (a NaN keeps its payload):
 * the bits of torch's max_pool2d on the 16-bit tensor.
 *
 * mhaq_fq_bn_pool_bwd_x16: mhaq_fq_bn_bwd_x16 on x[n, h, w, c] whose 16-bit dy is torch's max_pool2d backward of the 16-bit
 * pooled gradient g[n, oh, ow, c], computed on the fly and never stored, bit for bit:
 *   where ONE window covers (ih, iw):   dy = that window's g, unchanged (-0.0 stays -0.0), if its code names (ih, iw); +0.0 if not
 *   where two or four windows do:       dy = R16(0.0f + sum of up(g)), an fp32 sum over the covering windows whose code names
 *                                       (ih, iw), in ascending oh, then ascending ow, rounded to nearest-even ONCE
 *   on a 1 x 1 plane (h == w == 1):   dy = R16(0.0f + up(g)) or +0.0: NHWC and NCHW are the same memory there, torch takes its
 *                                       contiguous kernel, and that one sums and rounds even a single window's g
 * R16 is torch's own conversion: for fp16 the hardware's (NaN stays NaN, overflow gives +-inf), for bf16 its software
 * rounding, under which EVERY NaN sum becomes the quiet NaN 0x7FC0.  dy is upcast again, exactly, before it enters the fp64
 * sums and the dx expression of mhaq_fq_bn_bwd_x16.  Same partition, sums and workspace layout as
 * mhaq_fq_bn_bwd_x16(m = n * h * w): mhaq_fq_bn_pool_bwd_x16_workspace_bytes(n, h, w, c) equals
 * mhaq_fq_bn_bwd_x16_workspace_bytes(n * h * w, c), and dx, dweight, dbias and every byte of the workspace are what that call
 * gives on the materialized dy.
 * ---------------------------------------------------------------------- */
int mhaq_fq_maxpool3s2_fwd_x16(const void* t, void* p, uint8_t* code, int64_t n, int64_t h, int64_t w, int64_t c, int dtype,
                               void* stream);
size_t mhaq_fq_bn_pool_bwd_x16_workspace_bytes(int64_t n, int64_t h, int64_t w, int64_t c);
int mhaq_fq_bn_pool_bwd_x16(const void* x, const void* g, const uint8_t* code, const float* mean, const float* invstd,
                            const float* weight, void* dx, float* dweight, float* dbias, int64_t n, int64_t h, int64_t w,
                            int64_t c, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * The training stem's forward on 16-bit tensors without a stored BatchNorm output: the third launch of mhaq_fq_bn_fwd_x16 and
 * mhaq_fq_maxpool3s2_fwd_x16 in one.  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION stays 4; a caller discovers it by symbol.
 *   x               dense NHWC [n, h, w, c] of the type named by `dtype`; p [n, oh, ow, c] of the same type and code
 *                   [n, oh, ow, c] (one byte each) as in mhaq_fq_maxpool3s2_fwd_x16, with its limits and alignments: c % 8 == 0,
 *                   c <= 2^22, n * h * w < 2^31; x and p 16-byte aligned, code 8-byte aligned
 *   mean, invstd    fp32 [c], required: the batch statistics, as mhaq_fq_bn_fwd_x16 saves them (called with y == NULL it
 *                   computes them, and updates the running statistics, in two launches)
 *   weight, bias    fp32 [c], NULL = 1, 0; these four 4-byte aligned
 * Contract: p and code are, bit for bit, what mhaq_fq_maxpool3s2_fwd_x16 writes from the y that mhaq_fq_bn_fwd_x16 writes from
 * the same x, mean, invstd, weight and bias.  With a = weight * invstd (an fp32 product), every element of a window becomes
 *   y = R16((up(x) - mean) * a + bias)
 * in fp32, in this order, without contraction, rounded to nearest-even ONCE; the pool's selection runs on those ROUNDED values
 * (the in-range positions in kh, then kw order, from -inf, replaced on  val > max || isnan(val)), p keeps the chosen y's 16
 * bits, and the code 4 / code 9 rule is unchanged.  Pooling x and normalizing the winner is a different function: two x that
 * round to one y tie, and the first in-range position wins; weight < 0 reverses the order; weight == 0 ties every window.
 * Argument errors are returned before any launch, in mhaq_fq_maxpool3s2_fwd_x16's order with mean and invstd among the
 * required pointers: NULL pointers, then the dtype, then non-positive sizes (MHAQ_FQ_EINVAL); width and range
 * (MHAQ_FQ_EUNSUPPORTED); the alignment (MHAQ_FQ_EALIGN).  One launch, no workspace: stream-ordered, capture-safe, stateless.
 * ---------------------------------------------------------------------- */
int mhaq_fq_bn_norm_pool3s2_fwd_x16(const void* x, const float* mean, const float* invstd, const float* weight,
                                    const float* bias, void* p, uint8_t* code, int64_t n, int64_t h, int64_t w, int64_t c,
                                    int dtype, void* stream);

/* ------------------------------------------------------------------------
 * Eval-mode BatchNorm of a FROZEN network (a distillation teacher: parameters and running statistics fixed between calls)
 * with what follows it in a ResNet block, one launch per place.  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION stays 4; a caller
 * discovers these entry points by symbol.  Tensors are dense fp32 NHWC seen as [m][c]; m >= 1, c % 4 == 0 and c <= 2^22
 * (else MHAQ_FQ_EUNSUPPORTED); tensors and constant slabs 16-byte aligned (else MHAQ_FQ_EALIGN).  Argument errors are
 * returned before any launch, with mhaq_fq_bn_fwd's codes in its order: required pointers, positive sizes and a known mode
 * (MHAQ_FQ_EINVAL), width and range (MHAQ_FQ_EUNSUPPORTED), the alignment (there is no workspace).
 *
 * mhaq_fq_bn_infer_consts: consts[3][c] = {running_mean, a, bias} with a = weight * (running_var + eps)^-1/2 evaluated in
 * fp64 and rounded to fp32 ONCE; weight NULL = 1, bias NULL = 0.  The slab is the caller's; it is valid until a parameter,
 * a statistic or eps changes.
 *
 * mhaq_fq_bn_infer_act: with t = (x - mean) * a + bias in fp32, in this order, without contraction (mhaq_fq_bn_fwd's
 * expression), and relu(v) = v > 0 ? v : (isnan(v) ? v : 0):
 *   MHAQ_FQ_BN_RELU        y = relu(t)                x2, consts2, residual NULL
 *   MHAQ_FQ_BN_ADD_RELU    y = relu(t + residual)     residual [m][c] required; x2, consts2 NULL
 *   MHAQ_FQ_BN2_ADD_RELU   y = relu(t + t2)           t2 = the same expression of x2 [m][c] with consts2; residual NULL
 * (an operand the mode does not read, or a missing one: MHAQ_FQ_EINVAL).  The sum is rounded to fp32 before the ReLU: every
 * y is the bits of torch's separate sub, mul, add, add and relu on the same constants.  y must not overlap an input.
 *
 * mhaq_fq_bn_relu_pool3s2: p[n, oh, ow, c] = max_pool2d(relu(t), kernel 3, stride 2, padding 1) of x[n, h, w, c], t never
 * stored; geometry, limits (n * h * w < 2^31) and selection (start at -inf, replace on val > max || isnan(val)) are
 * mhaq_fq_maxpool3s2_fwd's.
 * Each is one launch: stream-ordered, no host synchronisation, capture-safe, stateless.
 * ---------------------------------------------------------------------- */
enum { MHAQ_FQ_BN_RELU = 0, MHAQ_FQ_BN_ADD_RELU = 1, MHAQ_FQ_BN2_ADD_RELU = 2 };
int mhaq_fq_bn_infer_consts(const float* running_mean, const float* running_var, const float* weight, const float* bias,
                            double eps, int64_t c, float* consts /* [3][c] */, void* stream);
int mhaq_fq_bn_infer_act(const float* x, const float* consts, const float* x2, const float* consts2, const float* residual,
                         float* y, int64_t m, int64_t c, int mode, void* stream);
int mhaq_fq_bn_relu_pool3s2(const float* x, const float* consts, float* p, int64_t n, int64_t h, int64_t w, int64_t c,
                            void* stream);

/* ------------------------------------------------------------------------
 * The same two launches on 16-bit tensors (the frozen network under torch.autocast).  Additive to ABI v4 --
 * MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.  x, x2, residual, y and p are dense NHWC tensors
 * of the type named by `dtype` (MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16, anything else: MHAQ_FQ_EINVAL); c % 8 == 0 and c <= 2^22
 * (else MHAQ_FQ_EUNSUPPORTED; the pool keeps n * h * w < 2^31); tensors and slabs 16-byte aligned (else MHAQ_FQ_EALIGN).  The
 * constant slabs are mhaq_fq_bn_infer_consts's fp32 [3][c], unchanged.  A mode's operands are required or refused as above.
 * Argument errors are returned before any launch, in the fp32 entry points' order with the dtype behind the NULL, size and
 * mode checks: required pointers, positive sizes, a known mode and its operands, the dtype (MHAQ_FQ_EINVAL); width and
 * range; the alignment.
 *
 * The arithmetic is the fp32 contract on the exactly upcast inputs, rounded ONCE to nearest-even at the end:
 *   y = R16(relu(fl32((up(x) - mean) * a + bias  [+ up(residual)]  [+ t2])))
 * uncontracted, in the fp32 order, the sum rounded to fp32 before the ReLU; relu keeps a NaN and a NaN stays a NaN in 16 bits
 * (its payload is not specified); an fp16 result beyond the fp16 range is +-inf, as a cast gives.
 *   p = R16(max_pool2d(relu(t), 3, 2, 1))  with mhaq_fq_maxpool3s2_fwd's selection on the fp32 values.
 * Each is one launch: stream-ordered, no host synchronisation, capture-safe, stateless.  y must not overlap an input.
 * ---------------------------------------------------------------------- */
int mhaq_fq_bn_infer_act_x16(const void* x, const float* consts, const void* x2, const float* consts2, const void* residual,
                             void* y, int64_t m, int64_t c, int mode, int dtype, void* stream);
int mhaq_fq_bn_relu_pool3s2_x16(const void* x, const float* consts, void* p, int64_t n, int64_t h, int64_t w, int64_t c,
                                int dtype, void* stream);

/* ------------------------------------------------------------------------
 * One-pass RAdam: the optimizer step of every parameter tensor of a model in ONE launch, with the bits of
 * torch.optim.RAdam(foreach=True) on the same device (weight_decay = 0, maximize off, not capturable).  Additive to ABI v4 --
 * MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.
 *
 * A descriptor names one tensor's four streams -- p, g = p.grad, m = exp_avg, v = exp_avg_sq: fp32, n elements each, dense,
 * all four in the SAME memory order, at least 4-byte aligned, p / m / v overlapping nothing -- and its two scalars, which the
 * host computes in double precision as _multi_tensor_radam's non-capturable branch does and rounds to fp32 once:
 *   c1 = float(unrect_step_size)   = -lr / bias_correction1 while rho_t <= 5, then 0
 *   c2 = float(bias_correction2)   = -0.0 while rho_t <= 5, then -sqrt(1 - beta2^t) * lr * rect / bias_correction1
 * Per element, in fp32, each line rounded once (sqrt and both divisions correctly rounded):
 *   m = lerp(m, g, w1)                  w1 = float(1 - beta1);  |w1| < 0.5 ? m + w1 * (g - m) : g - (g - m) * (1 - w1)
 *   v = v * beta2                       beta2 = float(beta2)
 *   v = v + w2 * (g * g)                w2 = float(1 - beta2)
 *   b = sqrt(v);  b = b + eps;  b = b / c2;  b = 1 / b;  b = b + c1
 *   p = p + m * b
 * "Rounded once" includes the framework's contractions, measured on the device against its foreach kernels (DESIGN
 * section 14): the multiply-adds of the lerp and of the second moment are FUSED -- m = fmaf(w1, g - m, m), or
 * m = fmaf(g - m, -(1 - w1), g) where |w1| >= 0.5 (the negation on the weight: a NaN g - m keeps its sign),
 * v = fmaf(w2, g * g, v) --, and the last line is fmaf(1, m * b, p) with the 1 a run-time operand, as the framework's
 * addcmul multiplies by its `value`: that rounds like p + m * b, and where p and m * b are both NaN it keeps the bits
 * (the sign) the framework keeps.  While c2 is -0.0 the chain runs through -inf and -0.0 to b = c1: plain IEEE
 * operations, nothing special-cased.  NaN and infinities propagate as in the framework's chain, bit for bit.
 *
 * Geometry: `work_device` lists the launch's blocks: block i updates chunk `chunk` -- elements [chunk * C, min(n, chunk * C +
 * C)), C = mhaq_fq_radam_chunk_elements() -- of tensor `tensor` of the table.  The host lists every chunk of every tensor
 * exactly once, in any order.  A chunk whose four addresses are 16-byte aligned moves 16 bytes per access, any other one
 * dwords.  An entry outside the table or the tensor is skipped.  No atomics, no workspace: 7 passes over the data.
 * Argument errors are returned before the launch: negative counts, NULL tables with work to do (MHAQ_FQ_EINVAL), more
 * than 2^31 - 1 blocks (MHAQ_FQ_EUNSUPPORTED), tables not 8-byte aligned (MHAQ_FQ_EALIGN); nwork == 0 is a valid empty step.
 * The tables are read by the kernel: they stay untouched until the launch has run.  Stream-ordered, no host
 * synchronisation, stateless.  (A CAPTURED launch would freeze c1 / c2, which change every step: step eagerly.)
 * ---------------------------------------------------------------------- */
typedef struct {
  float* p;        /* the parameter, updated in place */
  const float* g;  /* its gradient */
  float* m;        /* exp_avg, updated in place */
  float* v;        /* exp_avg_sq, updated in place */
  int64_t n;       /* elements */
  float c1, c2;    /* this tensor's scalars at its own step count */
} mhaq_radam_desc;
typedef struct {
  int32_t tensor;  /* index into the descriptor table */
  int32_t chunk;   /* chunk of that tensor */
} mhaq_radam_work;
int64_t mhaq_fq_radam_chunk_elements(void);
int mhaq_fq_radam_step(const mhaq_radam_desc* descs_device, int ntensors, const mhaq_radam_work* work_device,
                       int64_t nwork, float w1, float beta2, float w2, float eps, void* stream);

/* ------------------------------------------------------------------------
 * Distillation losses over two logit tensors: the six softmax-family losses a config can name (Cross-Entropy, Symmetrical
 * Cross-Entropy, KL, Symmetrical KL, JSD, Hellinger) in two launches forward and one backward.  Additive to ABI v4 --
 * MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.
 *   x, t          the student's and the teacher's logits, dense row-major [rows][cols]; each of them MHAQ_FQ_DT_F32,
 *                 MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16 (x_dtype, t_dtype; the two may differ), aligned to its element size.
 *                 16-bit elements are converted up exactly; everything else is fp32 arithmetic, reduced in fp64.
 *   kind          MHAQ_FQ_DISTILL_*
 *   loss          [1] fp32: sum of the terms below over all elements / denom, summed in fp64 and rounded once
 *   gunit         NULL, or [rows][cols] fp32: d loss / d x for an upstream gradient of 1
 *   workspace     mhaq_fq_distill_loss_workspace_bytes(rows) bytes, 8-byte aligned: one fp64 partial per row
 * With ps, pt = softmax(x), softmax(t) per row (row maximum subtracted), ls, lt the log-softmaxes, d = ls - lt,
 * B = rows, N = rows * cols and r_j = denom * gunit_j:
 *   CE         term -pt * ls             denom B    r_j = ps_j - pt_j
 *   SCE        term -pt * ls - ps * lt   denom B    r_j = ps_j - pt_j - ps_j * (lt_j - M),  M = sum_c ps_c * lt_c
 *   KL         term pt * (lt - ls)       denom N    r_j = ps_j - pt_j
 *   SKL        term (ps - pt) * d        denom B    r_j = ps_j - pt_j + ps_j * (d_j - K),   K = sum_c ps_c * d_c
 *   JSD        term (ps - pt) * d        denom 2N   r_j as SKL
 *   HELLINGER  term (sqrt ps - sqrt pt)^2  denom N  r_j = h_j - ps_j * H,  h = sqrt ps * (sqrt ps - sqrt pt),  H = sum_c h_c
 * A NaN or infinite logit makes its own row's partial and gunit row NaN (and so the loss) and leaves other rows' gunit
 * alone.  The same inputs give the same bits at every call: no atomics, fixed summation orders.
 * _fwd: launch one, one workgroup per row (rows of up to 4096 columns are held in registers, longer ones are walked
 * once per pass); launch two, one workgroup, sums the row partials.  _bwd: gx[i] = gunit[i] * g[0], rounded to nearest-
 * even once into gx_dtype (fp32, bf16 or fp16); g is read on the device, so a replayed hipGraph sees the current value.
 * Argument errors are returned before any launch: NULL x / t / loss / workspace (gunit / g / gx), rows, cols or n <= 0,
 * an unknown kind or dtype (MHAQ_FQ_EINVAL); a short workspace (MHAQ_FQ_EWORKSPACE); a pointer not aligned to its
 * element size (MHAQ_FQ_EALIGN); rows > 2^31 - 1 (MHAQ_FQ_EUNSUPPORTED).  Stream-ordered, no host synchronisation, stateless.
 * ---------------------------------------------------------------------- */
enum { MHAQ_FQ_DISTILL_CE = 0, MHAQ_FQ_DISTILL_SCE = 1, MHAQ_FQ_DISTILL_KL = 2,
       MHAQ_FQ_DISTILL_SKL = 3, MHAQ_FQ_DISTILL_JSD = 4, MHAQ_FQ_DISTILL_HELLINGER = 5 };
size_t mhaq_fq_distill_loss_workspace_bytes(int64_t rows);
int mhaq_fq_distill_loss_fwd(const void* x, int x_dtype, const void* t, int t_dtype,
                             int64_t rows, int64_t cols, int kind,
                             float* loss /* [1] */, float* gunit /* [rows*cols], nullable */,
                             void* workspace, size_t workspace_bytes, void* stream);
int mhaq_fq_distill_loss_bwd(const float* gunit, const float* g /* [1], device */,
                             void* gx, int gx_dtype, int64_t n, void* stream);

/* ------------------------------------------------------------------------
 * Classification head over one logit tensor and hard labels: the mean cross-entropy, the per-row nll, the rank of the
 * label's logit with the top-1 / top-k counts, and optionally the gradient, from one read of the logits in two launches.
 * The backward is mhaq_fq_distill_loss_bwd above (gx = RNE(gunit * g[0])).  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION stays
 * 4; a caller discovers these entry points by symbol.
 *   x             logits, dense row-major [rows][cols]; MHAQ_FQ_DT_F32, MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16, aligned to its
 *                 element size.  16-bit elements are converted up exactly; everything else is fp32 arithmetic (no
 *                 contraction, no approximate transcendentals), reduced in fp64.
 *   target        [rows] int64.  A row is VALID when target != ignore_index and 0 <= target < cols; V = number of valid rows.
 *                 A target that is neither ignore_index nor in range sets bit 2 of `flags` and its row is treated as ignored:
 *                 no address is ever formed from it (the framework's loss aborts the process with a device-side assert there).
 *   topk          >= 1; with topk >= cols every valid row counts
 *   loss          [1] fp32: (sum of nll over the valid rows) / V, summed in fp64 in a fixed order and rounded once; NaN for V = 0
 *   acc           [2] fp32: float(counts[1]) / float(V) and float(counts[2]) / float(V), one IEEE division each; 0 for V = 0
 *   counts        [3] int64: V, #{valid rows with rank == 0}, #{valid rows with rank < topk}
 *   nll           NULL, or [rows] fp32 (0 on rows that are not valid)
 *   rank          NULL, or [rows] int32 (cols on rows that are not valid)
 *   gunit         NULL, or [rows][cols] fp32: d loss / d x for an upstream gradient of 1; every element is written
 *   flags         [1] device word, WRITTEN by the call (not OR-ed into): bit 1 (value 2) = the nll of a valid row is not
 *                 finite, bit 2 (value 4) = a target out of range
 *   workspace     mhaq_fq_cls_head_workspace_bytes(rows) bytes, 8-byte aligned: per row an fp64 partial, the rank, a status
 * Per valid row with label y:  m = max_c x_c,  S = sum_c exp(x_c - m) (fp64 sum, rounded to fp32),
 *   nll = log S - (x_y - m)   (= lse - x_y with lse = m + log S, in the framework's order of operations),
 *   gunit_j = (exp(x_j - m) / S - [j == y]) / V;  gunit is 0 on every other row.
 * rank = the label's position in torch.sort(x, descending=True, stable=True):
 *   rank = #{c : x_c > x_y} + #{c < y : x_c == x_y},  where a NaN sorts above +inf and equals a NaN, and +0 == -0.
 * Hence argmax(x) == y exactly when rank == 0, ties and NaN rows included.
 * There is no other screening: a NaN or infinite logit spoils its own row's nll (and the loss) by plain IEEE arithmetic and
 * leaves the other rows' nll, rank and gunit bits alone.  The same inputs give the same bits at every call: no atomics,
 * fixed summation orders, no host synchronisation, no data-dependent host scalar; stream-ordered, capture-safe, stateless.
 * Launch one, one workgroup per row (rows of up to 4096 columns are held in registers, longer ones are walked once per
 * pass; with a gunit, each valid row's workgroup also counts V over `target` itself, rows * 8 bytes out of L2); launch two,
 * one workgroup, adds the rows up.
 * Argument errors are returned before any launch, in this order: NULL x / target / loss / acc / counts / flags / workspace,
 * rows or cols < 1, topk < 1, an unknown dtype (MHAQ_FQ_EINVAL); a short workspace (MHAQ_FQ_EWORKSPACE); x not aligned to
 * its element size, target / counts / workspace not 8-byte or another pointer not 4-byte aligned (MHAQ_FQ_EALIGN); rows or
 * cols > 2^31 - 1 (MHAQ_FQ_EUNSUPPORTED).
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_cls_head_workspace_bytes(int64_t rows);
int mhaq_fq_cls_head_fwd(const void* x, int x_dtype, const int64_t* target, int64_t rows, int64_t cols,
                         int64_t ignore_index, int topk,
                         float* loss /* [1] */, float* acc /* [2] */, int64_t* counts /* [3] */,
                         float* nll /* [rows], nullable */, int32_t* rank /* [rows], nullable */,
                         float* gunit /* [rows*cols], nullable */, uint32_t* flags /* [1] */,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Object-detection validation: the YOLO head's non-maximum suppression and COCO's greedy matching of its output against
 * the ground truth, in three entry points with the caller's sort between the first two.  Additive to ABI v4 --
 * MHAQ_FQ_ABI_VERSION stays 4; a caller discovers these entry points by symbol.
 *   pred          what the head returns in eval mode, dense [B][4 + nc][A]; MHAQ_FQ_DT_F32, MHAQ_FQ_DT_BF16 or MHAQ_FQ_DT_F16,
 *                 aligned to its element size.  Rows 0-3 are cx, cy, w, h in pixels, rows 4.. the class scores (already
 *                 sigmoided).  16-bit elements are converted up exactly; everything after that is fp32 arithmetic with no
 *                 contraction and IEEE division.
 * The contract restates the reference's non_max_suppression with its NMS call written out; it is not a recording.
 * Candidates.  Pair (a, c) is a candidate iff score[a][c] > conf_thr; a NaN score is never one.  conf_thr is finite and
 *   >= 0, so the bit pattern of every candidate's score is a non-negative int32.
 * Order.  Descending score, ties by (a, c) ascending (a stable descending sort of the reference's candidate list; the
 *   reference's own argsort leaves the order of ties undefined, so this is one of its valid results), realised as
 *   key = (int64(0x7FFFFFFF - bits(score)) << 32) | (a * nc + c);  a pair that is no candidate carries INT64_MAX.  Keys are
 *   unique, so ascending key order is the order.  Only the first max_nms candidates (reference: 30000) go on.
 * Boxes.  x1 = cx - w / 2, y1 = cy - h / 2, x2 = cx + w / 2, y2 = cy + h / 2.  The class offset is o = float(c) * max_wh
 *   (reference: 7680), the offset box b = box + o, each coordinate rounded once, and area = (b.x2 - b.x1) * (b.y2 - b.y1)
 *   is taken on the OFFSET box.  At class 79 the offset coordinates sit on a grid of 1/16 px: that is part of the contract.
 * Suppression.  Walk the candidates in order: candidate j is kept iff no earlier KEPT candidate i has
 *   inter / ((area_i + area_j) - inter) > iou_thr,  inter = max(0, min(i.x2, j.x2) - max(i.x1, j.x1)) * (the same in y),
 *   where min(p, q) = q < p ? q : p and max(p, q) = p < q ? q : p with p the kept box's operand (0 in the outer max): a NaN
 *   compares false.  The comparison is strict and in fp32; 0 / 0 is NaN and does not suppress.  The first max_det kept
 *   candidates (reference: 100) are the output, and the walk ends there.
 *
 * mhaq_fq_od_keys: one launch, one read of the score rows, coalesced along A.
 *   keys          [B][A * nc] int64, 8-byte aligned.  Every element is written; the POSITION of a key inside its image's row
 *                 is unspecified (the order lives in the key's value).  The caller sorts each row ascending (any sort of
 *                 int64 rows) before mhaq_fq_od_nms.
 *   Errors, before the launch: NULL pred / keys, an unknown dtype, B, nc or A < 1, conf_thr negative, NaN or infinite
 *   (MHAQ_FQ_EINVAL); pred not aligned to its element size, keys not 8-byte aligned (MHAQ_FQ_EALIGN); A * nc > 2^31 - 1,
 *   B or nc > 65535 (MHAQ_FQ_EUNSUPPORTED).
 *
 * mhaq_fq_od_nms: two launches (one workgroup per image; one workgroup for the flag word).
 *   keys          the rows of mhaq_fq_od_keys, each sorted ascending.  A key inside the candidate range whose low word is
 *                 not below A * nc is skipped; no address is formed from it.
 *   det           [B][max_det][6] fp32: x1, y1, x2, y2 of the UN-offset box, score, float(class), in kept order; rows at and
 *                 beyond count[b] are written as zeros
 *   count         [B] int32, kept boxes of the image (<= max_det)
 *   n_cand        [B] int32, candidates of the image before the truncation to max_nms: the position of the first INT64_MAX
 *                 of its sorted row (a binary search; no count kernel, no atomics)
 *   flags         [1] device word, WRITTEN by the call: bit 0 (value 1) = a NaN or infinite coordinate x1, y1, x2 or y2 of
 *                 the un-offset box among the candidates that were walked, i.e. those at sorted positions up to and including
 *                 the one that filled the list, or all of the first max_nms when the list did not fill; bit 1 (value 2) = an
 *                 image had more than max_nms candidates
 *   workspace     mhaq_fq_od_nms_workspace_bytes(B) bytes, 4-byte aligned: one flag word per image
 *   Workspace and LDS grow with B and max_det only, never with the square of the candidate count: mhaq_fq_od_nms_chunk()
 *   candidates at a time are tested against the kept boxes (LDS) and then resolved among themselves in order, a box being
 *   tested only against boxes that are kept.  Ending the walk at max_det is exact: whether a candidate is kept depends on
 *   earlier candidates only.  There is no wall-clock limit: every image of the batch is processed.
 *   Errors, before any launch: a NULL pointer, an unknown dtype, B, nc, A, max_nms or max_det < 1, iou_thr NaN, max_wh NaN or
 *   infinite (MHAQ_FQ_EINVAL); a short workspace (MHAQ_FQ_EWORKSPACE); pred not aligned to its element size, keys not 8-byte
 *   or another pointer not 4-byte aligned (MHAQ_FQ_EALIGN); A * nc > 2^31 - 1, B or nc > 65535, max_det > 1024
 *   (MHAQ_FQ_EUNSUPPORTED).
 *
 * mhaq_fq_od_match: COCO's greedy matching (pycocotools' evaluateImg for area = all, no crowd boxes, maxDets = max_det) of a
 * batch's detections against its ground truth, one launch, one workgroup of ten wavefronts per image.
 *   det, count    as written by mhaq_fq_od_nms (count is clamped to [0, max_det])
 *   nc            classes: a ground-truth label outside [0, nc) sets bit 2 (value 4) of flags; that box is ignored and no
 *                 address is formed from its label
 *   gt_box        [G][4] fp32 x1, y1, x2, y2;  gt_label [G] int64;  gt_off [B + 1] int64, CSR offsets of the images into
 *                 them (device memory; clamped to [0, G]).  G == 0: gt_box, gt_label and workspace may be NULL.
 *   tp            [B][max_det] int32: bit k = detection d is matched at threshold T_k; 0 at and beyond count[b]
 *   flags         [1] device word, OR-ed into (mhaq_fq_od_nms wrote it)
 *   workspace     mhaq_fq_od_match_workspace_bytes(G) bytes: one mark per ground-truth box and threshold
 *   Per image and k = 0..9, T_k = the fp64 values of numpy.linspace(0.5, 0.95, 10): detections are walked in output order;
 *   detection d of class c takes, among the image's ground truth with label c that is still unmatched at k and has
 *   double(iou32(d, g)) >= T_k, the one with the largest IoU, ties to the highest index (pycocotools' >= update rule);
 *   both are then marked.  iou32 is the formula above on the un-offset boxes (p the detection's operand), areas
 *   (x2 - x1) * (y2 - y1); a NaN never matches.
 *   Errors, before the launch: NULL det / count / gt_off / tp / flags, B, max_det or nc < 1, G < 0, with G > 0 a NULL gt_box /
 *   gt_label / workspace (MHAQ_FQ_EINVAL); a short workspace (MHAQ_FQ_EWORKSPACE); gt_label / gt_off not 8-byte or another
 *   pointer not 4-byte aligned (MHAQ_FQ_EALIGN); max_det > 1024 (MHAQ_FQ_EUNSUPPORTED).
 * All three: stream-ordered, capture-safe, stateless, no host synchronisation, no atomics (every word has one writer); the
 * same inputs give the same bits at every call.
 * ---------------------------------------------------------------------- */
int mhaq_fq_od_nms_chunk(void);
int mhaq_fq_od_keys(const void* pred, int pred_dtype, int64_t B, int64_t nc, int64_t A, float conf_thr,
                    int64_t* keys /* [B][A*nc] */, void* stream);
size_t mhaq_fq_od_nms_workspace_bytes(int64_t B);
int mhaq_fq_od_nms(const void* pred, int pred_dtype, const int64_t* keys /* sorted rows */,
                   int64_t B, int64_t nc, int64_t A, float iou_thr, float max_wh, int max_nms, int max_det,
                   float* det /* [B][max_det][6] */, int32_t* count /* [B] */, int32_t* n_cand /* [B] */,
                   uint32_t* flags /* [1] */, void* workspace, size_t workspace_bytes, void* stream);
size_t mhaq_fq_od_match_workspace_bytes(int64_t G);
int mhaq_fq_od_match(const float* det, const int32_t* count, int64_t B, int max_det, int64_t nc,
                     const float* gt_box /* [G][4] */, const int64_t* gt_label /* [G] */,
                     const int64_t* gt_off /* [B+1] */, int64_t G, int32_t* tp /* [B][max_det] */,
                     uint32_t* flags /* [1] */, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Super-resolution validation metrics: per-image PSNR and SSIM of the clamped prediction against the target and the L1
 * criterion on the unclamped one, in three launches.  Additive to ABI v4 -- MHAQ_FQ_ABI_VERSION stays 4; a caller discovers
 * these entry points by symbol.
 *   sr, hr        the model output s and the target h, dense NCHW [n][c][h][w]; each of them MHAQ_FQ_DT_F32, MHAQ_FQ_DT_BF16
 *                 or MHAQ_FQ_DT_F16 (the two may differ), aligned to its element size.  16-bit elements are converted up
 *                 exactly; everything else is fp32 arithmetic (no contraction), reduced in fp64.
 *   sr_div        s' = s / sr_div, an IEEE division (255 for a de-normalised model, else 1); finite and non-zero
 *   to_luminance  non-zero (c must be 3): ONE plane per image, x = (s''_R * k0 + s''_G * k1) + s''_B * k2 and y the same
 *                 from h, k = fp32([65.738, 129.057, 25.064]) / 256.  Zero: the c channels are the P = c planes.
 *   pool          the SSIM pool factor f >= 1; the reference's value is max(1, round(min(h, w) / 256)), halves to even
 *   psnr, ssim    [n] fp32;  l1 [1];  mean [2] = the batch means of PSNR and SSIM;  each summed in fp64 and rounded once
 *   flags         [1] device word, OR-ed into (the caller clears it): bit 0 = a NaN or an infinity in s' or h, bit 1 = a
 *                 target plane value outside [0, 1] (where a metrics library would refuse the input)
 *   workspace     mhaq_fq_sr_metrics_workspace_bytes(...) bytes, 8-byte aligned: the pooled planes xp, yp as fp32
 *                 [n][P][hp][wp] (hp = floor(h / f), wp = floor(w / f)) and the fp64 partials of the launches
 * Definitions.  l1 = mean |s' - h| over all elements, unclamped.  s'' = clamp(s', 0, 1) where a NaN stays a NaN; h is not
 * clamped.  PSNR of an image = -10 * log10(mean over its P * h * w plane values of (x - y)^2 + 1e-8): every pixel counts,
 * also the remainder rows and columns the pool drops.  SSIM of an image: the planes are average-pooled with kernel and
 * stride f in floor mode (f == 1: the planes themselves); G = the 11 x 11 Gaussian window, sigma 1.5, normalised to sum
 * 1, applied without padding; mx, my = G * x, G * y; sxx = G * x^2 - mx^2, syy likewise, sxy = G * (x y) - mx my;
 * c1 = 1e-4, c2 = 9e-4; cs = (2 sxy + c2) / (sxx + syy + c2); ss = (2 mx my + c1) / (mx^2 + my^2 + c1) * cs; SSIM = the
 * mean of ss over the (hp - 10) * (wp - 10) window positions and the planes.  x^2, y^2, x y and their filtered sums are
 * formed by the same operations in the same order, so s'' and h with equal bits give SSIM == 1.0f exactly.
 * A NaN in one image makes that image's PSNR and / or SSIM NaN (and l1 and the batch means) by plain IEEE arithmetic; the
 * other images' outputs keep their bits.  The same inputs give the same bits at every call: no atomics, fixed orders.
 * Launches: prepare (one read of s and h: the division, the |s' - h| and (x - y)^2 partials, the clamp, the planes, the
 * flags, the pooled planes), SSIM tiles (32 x 32 window positions of one plane per workgroup, separable filter in LDS, one
 * fp64 partial per workgroup), finalize (one workgroup).
 * Argument errors are returned before any launch, in this order: a NULL pointer; an unknown dtype; n, c, h, w <= 0,
 * pool < 1, sr_div not finite or zero; to_luminance with c != 3 (all MHAQ_FQ_EINVAL); a short workspace
 * (MHAQ_FQ_EWORKSPACE); sr / hr not aligned to their element size, an output or the workspace not 8-byte aligned
 * (MHAQ_FQ_EALIGN); floor(h / pool) < 11 or floor(w / pool) < 11 (no window fits), c not in {1, 3}, more partials than a
 * grid dimension allows (MHAQ_FQ_EUNSUPPORTED; _workspace_bytes returns 0 for every size the call refuses).
 * Stream-ordered, capture-safe, no host synchronisation, stateless.
 * ---------------------------------------------------------------------- */
size_t mhaq_fq_sr_metrics_workspace_bytes(int64_t n, int64_t c, int64_t h, int64_t w, int to_luminance, int pool);
int mhaq_fq_sr_metrics(const void* sr, int sr_dtype, const void* hr, int hr_dtype,
                       int64_t n, int64_t c, int64_t h, int64_t w, float sr_div, int to_luminance, int pool,
                       float* psnr /* [n] */, float* ssim /* [n] */, float* l1 /* [1] */, float* mean /* [2] */,
                       uint32_t* flags /* [1] */, void* workspace, size_t workspace_bytes, void* stream);

/* Whole-tensor min / max (zero point of a PER_TENSOR weight quantizer,
 * gdnsq_conv2d.py:82-83; min/max observer, calib/minmaxobserver.py:19-36).
 * out[0] = min, out[1] = max. */
size_t mhaq_fq_minmax_workspace_bytes(int64_t n);
int mhaq_fq_minmax(const float* x, int64_t n, float* out /* [2] */,
                   void* workspace, size_t workspace_bytes, void* stream);

/* Per-row min / max of W viewed as [co][row] (weight-scale calibration, calib/minmaxobserver.py:73-75:
 * weight.amax((1,2,3)) / amin((1,2,3))); NaN-propagating like torch.  Read-only, one workgroup per row. */
int mhaq_fq_row_minmax(const float* w, int64_t co, int64_t row, float* mn_out /* [co] */,
                       float* mx_out /* [co] */, void* stream);

/* amin backward for a PER_TENSOR weight (tie-split scatter):
 * gw[i] += [w[i] == *zp] * grads[1] / grads[4]   with grads from mhaq_fq_pt_bwd. */
int mhaq_fq_pt_tie_scatter(const float* w, float* gw, int64_t n, const float* zp,
                           const float* grads /* [5] */, void* stream);

/* AEWGS statistics for a PER_TENSOR scale: per position j in [0,row) the means
 * over the `co` rows of sign(G*s)*e, e^2, e  -> stats[3][row]  (gdnsq.py:118-124).
 * lo / hi: clamp bounds (NULL = unbounded, the weight case).  Tall tensors are summed in row chunks
 * (fp64 partials in `workspace`, fixed-order finalize); _workspace_bytes is 0 when one chunk suffices. */
size_t mhaq_fq_pt_aewgs_colstats_workspace_bytes(int64_t co, int64_t row);
int mhaq_fq_pt_aewgs_colstats(const float* w, const float* G, int64_t co, int64_t row,
                              const float* s, const float* zp, const float* lo, const float* hi,
                              float* stats, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * Per-channel weight fake-quant: W viewed as [co][row], one scale per row,
 * zero point = row minimum (gdnsq_conv2d.py:71-98).  One workgroup per
 * channel; the row is staged in LDS so HBM is read once.
 *
 * Forward:  zp[c] = min_j W[c][j];  Wq = q*s[c] + zp[c]  (q as above, no clamp)
 * ---------------------------------------------------------------------- */
int mhaq_fq_pc_fwd(const float* w, float* wq, float* zp_out /* [co] */, float* q_out /* nullable */,
                   const float* s /* [co] */, int64_t co, int64_t row, void* stream);

/* Backward given G = dL/dWq:
 *   gW = gv/s + [W == zp] * g_zp / count(W == zp)     (amin backward, tie split)
 *   g_s[c] = sum_c G*q - sum_c gv*(v/s) + noise_term
 * `stats` [3][co]: AEWGS group statistics (after the cross-rank all-reduce of
 * gdnsq.py:126-129); NULL = compute them in-kernel from this rank's data
 * (single-process semantics).  Ignored for other methods.
 * `gzp_extra` [co]: gradient reaching zp from other consumers of the zero point
 * (the quantized bias, gdnsq_conv2d.py:87); added before the tie split.  NULL = none. */
int mhaq_fq_pc_bwd(const float* w, const float* G, float* gw, float* g_s /* [co] */,
                   const float* s /* [co] */, const float* zp /* [co] */,
                   int64_t co, int64_t row, int method, const float* stats,
                   const float* gzp_extra /* nullable [co] */,
                   const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, void* stream);

/* The whole per-channel NoisyConv2d weight path of one layer from its LEARNABLE parameter
 * (gdnsq_conv2d.py:71-98) plus the layer's regulariser input of ModelHelper.get_model_values
 * (utils/model_helper.py:21-25,44), which shares the row min/max already in LDS:
 *   fwd:  s = exp2(log_s[c]);  zp = row min;  mx = row max;  wq as mhaq_fq_pc_fwd;
 *         lwq[c] = log2((mx - zp) + s)
 *   bwd:  as mhaq_fq_pc_bwd, plus the gradient g_lwq of lwq: t = g_lwq / (((mx-zp)+s) * ln2) goes
 *         +t to the row maxima and -t to the row minima of gw (amax / amin backward, tie split)
 *         and +t to s;  g_log_s[c] = (dL/ds) * s * ln2   (exp2 backward).  g_lwq may be NULL. */
int mhaq_fq_wlayer_fwd(const float* w, float* wq, const float* log_s /* [co] */, int64_t co, int64_t row,
                       float* s_out, float* zp_out, float* mx_out, float* lwq_out /* [co] each */,
                       void* stream);
int mhaq_fq_wlayer_bwd(const float* w, const float* G, float* gw, float* g_log_s /* [co] */,
                       const float* s, const float* zp, const float* mx, const float* g_lwq /* nullable */,
                       int64_t co, int64_t row, int method, const float* stats,
                       const float* gzp_extra, const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                       void* stream);

/* The same for a PER_TENSOR layer small enough (n <= mhaq_fq_wlayer_pt_max_elements() = 64 K: every
 * CIFAR ResNet-20 / RFDN layer) for one workgroup: one launch per direction instead of
 * minmax + finalize + forward (+ torch's exp2 / amin / amax / log2 chain).  aux[4] = {s, zp, max, lwq}
 * (written by fwd, read by bwd); g_log_s[1]; g_lwq points at one float or is NULL.
 * method: STE, LSQ or EWGS (AEWGS' per-position statistics keep the general path). */
int64_t mhaq_fq_wlayer_pt_max_elements(void);
int mhaq_fq_wlayer_pt_fwd(const float* w, float* wq, const float* log_s /* [1] */, int64_t n,
                          float* aux /* [4] */, void* stream);
int mhaq_fq_wlayer_pt_bwd(const float* w, const float* G, float* gw, float* g_log_s /* [1] */,
                          const float* aux, const float* g_lwq, int64_t n, int method,
                          const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, void* stream);

/* The same for a PER_TENSOR layer of ANY size (e.g. ResNet-18 with `qscheme: 0`: up to 2.36 M weights per layer; and
 * every PER_TENSOR AEWGS layer -- the reference's default NoisyConv2d arguments, gdnsq_conv2d.py:27-32), as streaming
 * launches: fwd = min / max sweep -> scalar chain -> quantizer (3 launches); bwd = streaming backward with both tie
 * counts -> fixed-order sums -> scalar chain -> tie-split scatter to the minima AND maxima (4 launches).  Replaces
 * gdnsq_conv2d.py:72,82-83,96-98 and, for the regulariser input, model_helper.py:36-37,44 (torch amin / amax over the
 * weight again, and their autograd scatter).
 *   aux[7] = {s, zp = min, max, lwq = log2((max - min) + s), -inf, +inf, the backward's hi}   (written by fwd, read by bwd)
 *   bwd: g_log_s[1] = (dL/ds + t) * s * ln2 with t = g_lwq / (((max - min) + s) * ln2);
 *        gw = gv/s + [w == min] * (dL/dzp - t) / count(min) + [w == max] * t / count(max);  g_lwq nullable [1].
 *   AEWGS: `col_stats` [3][period] from mhaq_fq_pt_aewgs_colstats(w, G, co, period, aux, aux + 1, NULL, NULL, ...)
 *        (after the cross-rank all-reduce under data parallelism); NULL / 0 for the other estimators.
 *   workspace: mhaq_fq_wlayer_ptl_workspace_bytes(n) for both directions. */
size_t mhaq_fq_wlayer_ptl_workspace_bytes(int64_t n);
int mhaq_fq_wlayer_ptl_fwd(const float* w, float* wq, const float* log_s /* [1] */, int64_t n, float* aux /* [7] */,
                           void* workspace, size_t workspace_bytes, void* stream);
int mhaq_fq_wlayer_ptl_bwd(const float* w, const float* G, float* gw, float* g_log_s /* [1] */,
                           const float* aux /* [7] */, const float* g_lwq /* nullable [1] */, int64_t n, int method,
                           const float* col_stats, int64_t period,
                           const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Multi-tensor variants: every PER_CHANNEL weight layer of a model in ONE launch per direction, driven by
 * a device-resident pointer table.  Layer L owns channels [chan_offset, chan_offset + co) of the
 * per-channel slabs and elements [elem_offset, elem_offset + co*row) of the element slabs; the grid has
 * total_co workgroups.  aux_all is [4][total_co] = {s, zp, max, lwq} rows (written by fwd, read by bwd).
 * bwd reads G / g_lwq through the table (they arrive as separate autograd tensors) and writes gw_all
 * (element slab) and g_log_s_all [total_co].  stats_all: NULL or [3][total_co] AEWGS statistics.
 * Random signs: element e of layer L uses index elem_offset + e of the (seed, offset) stream.
 * The table's layers are listed in ascending chan_offset; every pointer in it (like every pointer of this header)
 * addresses device-visible GLOBAL memory -- the kernels read the rows through the global address space. */
typedef struct {
  const float* w;      /* [co][row] */
  const float* log_s;  /* [co] */
  const float* G;      /* bwd only */
  const float* g_lwq;  /* bwd only, nullable */
  int64_t co, row;
  int64_t elem_offset;
  int64_t chan_offset;
} mhaq_wlayer_desc;
int mhaq_fq_wlayer_fwd_multi(const mhaq_wlayer_desc* descs_device, int nlayers, int64_t total_co,
                             int64_t max_row, float* wq_all, float* aux_all, void* stream);
int mhaq_fq_wlayer_bwd_multi(const mhaq_wlayer_desc* descs_device, int nlayers, int64_t total_co,
                             int64_t max_row, const float* aux_all, float* gw_all, float* g_log_s_all,
                             int method, const float* stats_all, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                             void* stream);

/* The same backward for a GROUP of consecutive layers -- what a data-parallel trainer wants: the weight
 * gradients of a group leave together as soon as its last dL/dWq has arrived (gradient all-reduce overlap is
 * kept, unlike the model-wide launch), and AEWGS exchanges ONE packed [3][group_co] message per group instead of
 * one per layer (gdnsq.py:126-129 issues three per layer).  `descs_device` holds the group's layers with
 * chan_offset / elem_offset RELATIVE to the group (first layer: 0); `aux` points at the group's first channel in
 * row 0 of the forward's [4][aux_stride] slab (aux_stride = the model-wide total_co of mhaq_fq_wlayer_fwd_multi,
 * or group_co for a slab of the group's own); gw [group elements], g_log_s [group_co] and stats [3][group_co]
 * (nullable) are the group's own.  Sign stream: element e of the group uses index e of (seed, offset).
 * _aewgs_stats_group writes stats[3][group_co] = {mean sign(G*s)*e, mean e^2, mean e} of every channel of the
 * group in one launch (reads G through the table). */
int mhaq_fq_wlayer_bwd_group(const mhaq_wlayer_desc* descs_device, int nlayers, int64_t group_co, int64_t max_row,
                             const float* aux, int64_t aux_stride, float* gw, float* g_log_s, int method,
                             const float* stats, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                             void* stream);
int mhaq_fq_wlayer_aewgs_stats_group(const mhaq_wlayer_desc* descs_device, int nlayers, int64_t group_co,
                                     const float* aux, int64_t aux_stride, float* stats /* [3][group_co] */,
                                     void* stream);

/* ABI v4 -- Quantizer.quantize (gdnsq.py:189-219) of a [co][row] tensor with GIVEN per-row scale and zero point (bounds
 * -inf / +inf as for every weight quantizer, gdnsq_conv2d.py:76-77): q_out = rounding indices, y_out (nullable) =
 * q * s + zp.  The stand-alone facade on a weight -- utils/model_stats.py:118,123 quantizes the detached weights with the
 * zero point the layer's last forward left in Q, which mhaq_fq_pc_fwd (zero point = the row minimum it finds) cannot do.
 * flags: nullable int32[1] ZEROED by the caller; the kernel ORs MHAQ_FQ_FLAG_NOT_INTEGER into it (the only eval assert of
 * gdnsq.py:211-217 that can fire with infinite bounds).  Any row length / 4-byte alignment. */
int mhaq_fq_pc_quantize(const float* x, float* q_out, float* y_out, const float* s /* [co] */,
                        const float* zp /* [co] */, int64_t co, int64_t row, int32_t* flags, void* stream);

/* AEWGS per-channel statistics -> stats[3][co] = {mean sign(G*s)*e, mean e^2, mean e}. */
int mhaq_fq_pc_aewgs_stats(const float* w, const float* G, const float* s, const float* zp,
                           int64_t co, int64_t row, float* stats, void* stream);

/* ------------------------------------------------------------------------
 * Per-element parameters: x[i] quantized with s[i], zp[i] (no clamp) -- the
 * quant_bias=True branch of gdnsq_conv2d.py:86-94, where the bias reuses the
 * weight's per-channel scale and zero point.  n = C_out (small).
 *   fwd:  y = q*s + zp                      (q_out nullable)
 *   bwd:  gx = gv/s;  g_s[i] = g*q - gv*(v/s) + noise;  g_zp[i] = g - gv/s
 * AEWGS needs `stats` [3] = means over all n elements (reduce_to_shape with no
 * unit dimension reduces everything, gdnsq.py:150-152) from *_vec_aewgs_stats.
 * ---------------------------------------------------------------------- */
int mhaq_fq_vec_fwd(const float* x, float* y, float* q_out, const float* s, const float* zp, int64_t n,
                    void* stream);
int mhaq_fq_vec_aewgs_stats(const float* x, const float* g, const float* s, const float* zp, int64_t n,
                            float* stats /* [3] */, void* stream);
int mhaq_fq_vec_bwd(const float* x, const float* g, float* gx, float* g_s, float* g_zp,
                    const float* s, const float* zp, int64_t n, int method, const float* stats,
                    const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev, void* stream);

/* ------------------------------------------------------------------------
 * The reference's custom autograd Functions themselves, for callers that use
 * Quantizer.quantize / dequantize / _get_rnoise separately (the unfused
 * facade; utils/model_stats.py:116-132):
 *   noise_fwd   QNoise.forward (gdnsq.py:14-16):  out = rne(v) - v
 *   noise_bwd   QN{STE,LSQ,EWGS,AEWGS}.backward (gdnsq.py:35-147) given g = dL/dnoise:
 *               gv = estimator term, gs[group] = sum over the group of the
 *               scale-gradient terms.  `groups` scales own `len` consecutive
 *               elements each (1 = per-tensor, C_out = per-channel).
 *               AEWGS `stats`: [3][groups] (period == 0) or per position
 *               [3][period] (period > 0: the [1]-shaped-scale quirk), e.g. from
 *               mhaq_fq_pc_aewgs_stats / mhaq_fq_pt_aewgs_colstats with s = 1, zp = 0.
 * ---------------------------------------------------------------------- */
int mhaq_fq_noise_fwd(const float* v, float* out, int64_t n, void* stream);
size_t mhaq_fq_noise_bwd_workspace_bytes(int64_t groups, int64_t len);
int mhaq_fq_noise_bwd(const float* v, const float* g, float* gv, float* gs /* [groups] */,
                      int64_t groups, int64_t len, int method, const float* stats, int64_t period,
                      const int8_t* r_sign, uint64_t seed, uint64_t offset, const uint64_t* offset_dev,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------
 * PotentialLoss / PotentialLossNoPred arithmetic (gdnsq_loss.py:47-71, 129-153) over the concatenated
 * regulariser vectors las/laq [na] and lws/lwq [nw], one workgroup:
 *   hinge_w = max(0, (lwq-lws) - (w_bits - 1e-3))^p, hinge_a likewise with a_bits;
 *   ploss = (loss_sum/cnt * l1) * (wmul*mean hinge_w + amul*mean hinge_a) + l2 * base^p,
 *   (l1, l2) = (t, 1) or, lossless, (1, t);  wmul/amul from the counts of active hinges.
 *   The module state lives on the device: state[3] = {loss_sum, cnt, t} (running sum of the task loss, its
 *   step count, the temperature), so that a captured hipGraph sees their current values at every replay.
 *   fwd: out[12] = {ploss, wloss, aloss, rloss, cw, ca, cb, -mean lws, mean lwq, -mean las, mean laq,
 *        max(lwq-lws)};  update_state != 0 also does loss_sum += base^p, cnt += 1 (training mode).
 *   bwd: given g = dL/dploss [1] and `out` from fwd: g_base [1], g_las/g_laq [na], g_lws/g_lwq [nw].
 *   No NaN screening, plain IEEE as the reference (torch.max(0, h), .mean(), (lwq-lws).max()): a NaN in lws or lwq
 *   makes ploss, wloss, that vector's mean and max(lwq-lws) NaN, one in las or laq makes ploss, aloss and that
 *   vector's mean NaN; a NaN hinge counts as inactive (NaN > 0 is false).  The other side's outputs are untouched.
 *   The gradients under a NaN input are finite or NaN, not specified (the reference's own come from max's backward).
 * ---------------------------------------------------------------------- */
int mhaq_fq_potential_loss_fwd(const float* base, const float* las, const float* laq, int64_t na,
                               const float* lws, const float* lwq, int64_t nw,
                               float a_bits, float w_bits, float p, int lossless,
                               float* state /* [3] device, in/out */, int update_state,
                               float* out /* [12] */, void* stream);
int mhaq_fq_potential_loss_bwd(const float* g, const float* out, const float* las, const float* laq, int64_t na,
                               const float* lws, const float* lwq, int64_t nw,
                               float a_bits, float w_bits, float p,
                               float* g_base, float* g_las, float* g_laq, float* g_lws, float* g_lwq,
                               void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MHAQ_FQ_H */
