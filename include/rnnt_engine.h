/*
 * rnnt_engine.h — C ABI of librnnt_engine.so, the MI355X (gfx950) RNN-T joint + transducer
 * loss engine.  Plain pointers and sizes only; no torch types cross this boundary.
 *
 * The reference (jakepoz/rnnt) has NO native/FFI layer: its boundary for this path is the
 * Python pair
 *     rnnt.joint.JointNetwork.forward            /root/reference/rnnt/joint.py:25-39
 *     torchaudio.functional.rnnt_loss(...)       /root/reference/rnnt/model.py:35-41
 * followed by loss.backward()                    /root/reference/rnnt/train.py:133-134.
 * Each entry point below names the reference interface it replaces.  The Python host side
 * (rnnt_amd/engine.py) binds these symbols with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated otherwise; the caller owns all
 *     memory (inputs, outputs, workspace); the library never allocates or frees device
 *     memory and keeps no pointer after a call returns;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and returns without synchronising;
 *   - return value 0 = success, negative = error (RNNT_ERR_*); the message is available
 *     from rnnt_engine_last_error() (thread-local);
 *   - lattice layout: logits [B,T,U1,V] row-major contiguous, U1 = max target length + 1;
 *     targets [B,U1-1] int32, blank never appears in targets; lengths int32 [B];
 *   - precondition on the lengths (torchaudio checks the same on the host): 1 <= logit_lens[b] <= T,
 *     0 <= target_lens[b] <= U1-1.  The kernels CLAMP what they read into those ranges, so a
 *     violated precondition gives the loss of the clamped lattice, never an out-of-bounds access;
 *   - the library keeps no mutable state besides the thread-local error string; the device the
 *     pointers live on must be the calling thread's current HIP device.
 */
#ifndef RNNT_ENGINE_H
#define RNNT_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNNT_ENGINE_VERSION 4

#define RNNT_DTYPE_F32 0 /* fp32 in, fp32 MFMA (v_mfma_f32_32x32x2_f32), fp32 out */
/* BASELINE config 3 ("bf16"): pointers stay fp32 at this boundary (inputs, parameters, costs,
 * gradients); the operands of the three GEMMs — tanh(enc+pred), W and the logits gradient —
 * are rounded to bf16 (nearest-even) and multiplied by v_mfma_f32_32x32x16_bf16 with fp32
 * accumulation; the logits are kept in fp16 (workspace only; nearest-even, the loss is computed
 * from the stored values); log-softmax, the lattice and every reduction stay fp32/fp64.  Fused
 * entry only (rnnt_engine_joint_loss_fwd_bwd, rnnt_engine_run_stage, the workspace queries);
 * needs H % 128 == 0, V % 128 == 0. */
#define RNNT_DTYPE_BF16 1
/* fp32-ACCURATE arithmetic on the bf16 matrix pipes ("bf16x3"): same boundary, same 1e-4 parity bar as
 * RNNT_DTYPE_F32 — every operand of the three GEMMs is split once into three bf16 pieces (hi + mid + lo
 * = the fp32 value to 2^-25) and each product is the sum of six bf16 MFMA products with fp32 accumulation
 * (rnnt_amd/csrc/x3.hip); logits stay fp32, log-softmax / lattice / reductions are the fp32 route's.
 * Measured error against fp64 is below the fp32 MFMA route's (tools/bf16x3_accuracy.py, tests).  Fused
 * entry only; needs H % 128 == 0, V % 128 == 0 (the Python host side zero-pads other shapes). */
#define RNNT_DTYPE_F32_BF16X3 2
/* fp32-CLASS arithmetic on the fp16 matrix pipes at HALF the matrix work of RNNT_DTYPE_F32_BF16X3 ("f16x2", round 4): the
 * three bf16x3 GEMM kernels turned out power-bound (the chip holds 1.7-2.1 GHz under their MFMA stream), so the remaining
 * lever is fewer products.  Every operand of the three GEMMs is scaled by a power of two into fp16's range and split into
 * TWO fp16 pieces (hi + mid = the value to 2^-22: 11 + 11 significant bits); a product is the sum of THREE fp16 MFMA
 * products (hi.hi + hi.mid + mid.hi, fp32 accumulation) — rnnt_amd/csrc/x2.hip.  Same boundary, same 1e-4 parity bar, same
 * stages, variants and workspace objects as the bf16x3 route (no third plane); measured error against fp64: tests/test_x2_gpu.py.
 * Fused entry only; needs H % 128 == 0, V % 128 == 0. */
#define RNNT_DTYPE_F32_F16X2 3

#define RNNT_OK 0
#define RNNT_ERR_INVALID_ARG (-1) /* null pointer, non-positive dim, bad blank ...        */
#define RNNT_ERR_UNSUPPORTED (-2) /* dims the kernels do not cover (H%4, V%4, U1>1024 ...) */
#define RNNT_ERR_WORKSPACE (-3)   /* workspace too small                                   */
#define RNNT_ERR_LAUNCH (-4)      /* HIP reported an error at launch                       */

/* Library version (RNNT_ENGINE_VERSION it was built with). */
int rnnt_engine_version(void);

/* Diagnostic builds only (make EXTRA=-DRNNT_ABLATE / -DRNNT_STAMPS): process-wide ablation switches
 * of tools/exp_*.py and the device buffer of the in-kernel time stamps.  In the shipped library
 * both are no-ops (set_flags returns 0) — it has no global mutable state; alternative kernel
 * variants are chosen per call through rnnt_engine_run_stages. */
int rnnt_engine_set_flags(int flags);
void rnnt_engine_set_debug(void *buf);

/* Kernel variants a caller may ask for per call (rnnt_engine_run_stages).  Every variant multiplies
 * the same numbers in the same order as the default kernels: results are bit-identical. */
#define RNNT_VARIANT_SEPARATE_G 32          /* G by its own pass (k_make_g); the dHidden kernels read it    */
#define RNNT_VARIANT_SEPARATE_HIDDEN 64     /* hidden by its own pass instead of the forward prologue       */
#define RNNT_VARIANT_FWD_LDS_RING 128       /* forward main loop: W through an LDS-DMA ring                 */
#define RNNT_VARIANT_FWD_ONE_WG_PER_TILE 256 /* forward: one workgroup per tile instead of persistent ones   */
/* RNNT_DTYPE_F32_BF16X3 only: run one stage on the fp32 route's kernel instead of the bf16x3 one (same data
 * layout downstream, plain splitting kernels in between) — how each bf16x3 kernel is checked in isolation.
 * NOT bit-identical to the default bf16x3 kernels (different summation), same tolerance. */
#define RNNT_VARIANT_X3_FP32_FWD 4096       /* forward GEMM + hidden by the fp32 kernel, then k_split_make_hidden */
#define RNNT_VARIANT_X3_FP32_DH 8192        /* dHidden + G by the fp32 kernels, then k_split_g (needs _FWD too) */
/* RNNT_DTYPE_F32_F16X2 only: switch the flush rule off for this call.  By default that route gives every lattice cell whose
 * gradient row its fp16 split provably rounds to zero (|g_scale G| < 2^-26: rnnt_amd/csrc/lattice.hip k_coef, x2.hip) the
 * coefficients of a cell outside the lattice; dHidden tiles and 16-cell dW k-steps without a live cell are then skipped.  With this
 * bit no cell is flagged: tiles and k-steps are skipped by the utterances' lengths only.  costs, grad_enc and grad_pred are
 * bit-identical with and without it; grad_W / grad_bias differ in summation order only (the split-K ranges cut the list of live
 * k-steps at other cells).  The regularised entry (rnnt_engine_joint_loss_fwd_bwd_reg) always runs as if the bit were set:
 * the bound is not extended to FastEmit's / the delay penalty's coefficients. */
#define RNNT_VARIANT_X2_NO_FLUSH_SKIP 512
/* Bits 14 and up are reserved (they once named experimental kernels that have left the tree): every entry point that takes a
 * variant answers any of them with RNNT_ERR_UNSUPPORTED before it launches anything. */
#define RNNT_VARIANT_LAB_MASK 0x7fffc000

/* Diagnostic queries (0/1: predicted resident forward-kernel workgroups per CU). */
int rnnt_engine_debug_query(int what);

/* Message of the last error on the calling thread ("" if none). */
const char *rnnt_engine_last_error(void);

/* Bytes of device workspace rnnt_engine_joint_loss_fwd_bwd needs for these dims.  The workspace is
 * scratch: it need not be initialised (any bit pattern, NaNs included, is fine) and carries no
 * state from one call to the next. */
int rnnt_engine_workspace_bytes(int B, int T, int U1, int H, int V, int dtype, size_t *out);

/* Bytes of device workspace rnnt_engine_loss_fwd_bwd needs for these dims. */
int rnnt_engine_loss_workspace_bytes(int B, int T, int U1, int V, int dtype, size_t *out);

/* Bytes of device workspace rnnt_engine_joint_fwd needs for these dims. */
int rnnt_engine_joint_fwd_workspace_bytes(int B, int T, int U1, int H, int V, int dtype,
                                          size_t *out);

/*
 * logits[b,t,u,:] = tanh(enc[b,t,:] + pred[b,u,:]) @ W^T + bias
 * Replaces JointNetwork.forward's last three statements, reference rnnt/joint.py:32-39
 * (the optional audio_ln/text_ln projections of joint.py:26-30 stay with the caller).
 *   enc   [B,T,H] with element strides enc_strides[3] (the reference hands a permuted,
 *         non-contiguous view: rnnt/model.py:28); pred [B,U1,H] contiguous;
 *   W     [V,H] (torch.nn.Linear layout, joint.py:18); bias [V]; logits [B,T,U1,V] out.
 */
int rnnt_engine_joint_fwd(const void *enc, const int64_t enc_strides[3], const void *pred,
                          const void *W, const void *bias, int B, int T, int U1, int H, int V,
                          int dtype, void *logits, void *workspace, size_t ws_bytes,
                          void *stream);

/*
 * Transducer loss on given logits: per-utterance costs and d cost_b / d logits.
 * Replaces torchaudio.functional.rnnt_loss as called at reference rnnt/model.py:35-41
 * (fused log-softmax; `blank` already resolved to [0,V); clamp <= 0 means off).
 *   costs [B] out; grad_logits [B,T,U1,V] out or NULL (costs only).
 * Gradients are those of sum_b costs[b] (i.e. unscaled, as torchaudio stores them);
 * the caller applies the reduction / upstream factor.
 */
int rnnt_engine_loss_fwd_bwd(const void *logits, const int32_t *targets,
                             const int32_t *logit_lens, const int32_t *target_lens, int B,
                             int T, int U1, int V, int blank, float clamp, int dtype,
                             float *costs, void *grad_logits, void *workspace, size_t ws_bytes,
                             void *stream);

/*
 * Fused joint + transducer loss, forward AND backward in one call: everything between
 * `self.joint(...)` (reference rnnt/model.py:32) and the gradients loss.backward()
 * (rnnt/train.py:134) delivers to the joint's inputs and parameters.
 *   costs     [B]       per-utterance negative log-likelihood (fp32)
 *   grad_enc  [B,T,H]   contiguous, d(mean_b costs)/d enc     (reduction="mean", model.py:41)
 *   grad_pred [B,U1,H]  d(mean)/d pred
 *   grad_W    [V,H]     d(mean)/d W        grad_bias [V]  d(mean)/d bias
 * `grad_scale` multiplies every gradient (1/B for reduction="mean" on one device, 1/B_global
 * when the batch is sharded over ranks).  The (B,T,U1,V) logits live only in `workspace`.
 */
int rnnt_engine_joint_loss_fwd_bwd(const void *enc, const int64_t enc_strides[3],
                                   const void *pred, const void *W, const void *bias,
                                   const int32_t *targets, const int32_t *logit_lens,
                                   const int32_t *target_lens, int B, int T, int U1, int H,
                                   int V, int blank, float clamp, float grad_scale, int dtype,
                                   float *costs, void *grad_enc, void *grad_pred, void *grad_W,
                                   void *grad_bias, void *workspace, size_t ws_bytes,
                                   void *stream);

/*
 * Forward only: the per-utterance costs of the fused path and nothing else (no coefficient, dHidden
 * or dW kernels, no gradient buffers).  What `RNNTModel.forward` costs under torch.no_grad() —
 * the validation loss of reference rnnt/train.py:170-201 / rnnt/model.py:32-41.  Same workspace size
 * as rnnt_engine_joint_loss_fwd_bwd.
 */
int rnnt_engine_joint_loss_fwd(const void *enc, const int64_t enc_strides[3], const void *pred,
                               const void *W, const void *bias, const int32_t *targets,
                               const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                               int U1, int H, int V, int blank, int dtype, float *costs,
                               void *workspace, size_t ws_bytes, void *stream);

/*
 * Latency regularisers: the three loss entries above with FastEmit's lambda and
 * the delay penalty delta added; same workspace as their counterparts.  Both must be finite and
 * >= 0 (else RNNT_ERR_INVALID_ARG before anything is enqueued); at lambda = delta = 0 each launches
 * exactly its counterpart's kernels.  Per utterance, T_b / U_b clamped as everywhere:
 *   delay penalty: the lattice runs on lp_emit'(t,u) = lp_emit(t,u) + delta ((T_b - 1) / 2 - t)
 *                  (k2's definition); costs[b] = -log P'_b of that lattice, gradients its exact ones.
 *   FastEmit:      d/d logits gains lambda E(t,u) (p_k - [k = y_{u+1}]) for u < U_b, with
 *                  E = exp(alpha + lp_emit' + beta(t,u+1) - log P'_b) the label arc's occupancy (as
 *                  NeMo's warp-transducer kernel).  The reported cost does NOT change with lambda:
 *                  FastEmit is defined by its gradient, so costs stay comparable across lambda.
 * `clamp` (loss entry) applies to the final, regularised gradient.  The stage runner
 * (rnnt_engine_run_stage(s)) never applies either option.
 */
int rnnt_engine_loss_fwd_bwd_reg(const void *logits, const int32_t *targets,
                                 const int32_t *logit_lens, const int32_t *target_lens, int B,
                                 int T, int U1, int V, int blank, float clamp,
                                 float fastemit_lambda, float delay_penalty, int dtype,
                                 float *costs, void *grad_logits, void *workspace,
                                 size_t ws_bytes, void *stream);
int rnnt_engine_joint_loss_fwd_bwd_reg(const void *enc, const int64_t enc_strides[3],
                                       const void *pred, const void *W, const void *bias,
                                       const int32_t *targets, const int32_t *logit_lens,
                                       const int32_t *target_lens, int B, int T, int U1, int H,
                                       int V, int blank, float clamp, float grad_scale,
                                       float fastemit_lambda, float delay_penalty, int dtype,
                                       float *costs, void *grad_enc, void *grad_pred,
                                       void *grad_W, void *grad_bias, void *workspace,
                                       size_t ws_bytes, void *stream);
int rnnt_engine_joint_loss_fwd_reg(const void *enc, const int64_t enc_strides[3], const void *pred,
                                   const void *W, const void *bias, const int32_t *targets,
                                   const int32_t *logit_lens, const int32_t *target_lens, int B,
                                   int T, int U1, int H, int V, int blank, float delay_penalty,
                                   int dtype, float *costs, void *workspace, size_t ws_bytes,
                                   void *stream);

/*
 * Alignment-restricted loss, "Ar-RNN-T" (DESIGN.md §4n): the three *_reg entries above with the label arcs confined to a
 * window around a reference alignment; same workspace and return codes as their counterparts.
 *   restrict_frames [B, U1-1] int32, device, contiguous: the reference frame of every label, as rnnt_engine_align /
 *       rnnt_engine_joint_align write it; entries at u >= target_lens[b] are never read.  NULL: RNNT_ERR_INVALID_ARG.
 *   restrict_left, restrict_right >= 0 (else RNNT_ERR_INVALID_ARG), in encoder frames.
 * The label arc (t,u) -> (t,u+1) exists only for restrict_frames[b,u] - restrict_left <= t <= restrict_frames[b,u] +
 * restrict_right; blank arcs are unrestricted.  costs[b] = -log of the sum over the paths that remain, the gradients are that
 * cost's; a lattice cell no surviving path crosses contributes exactly zero.  FastEmit and the delay penalty act on the arcs
 * that remain.  An utterance without a surviving path (frames that decrease, or lie outside [0, T_b - 1] by more than the
 * buffers) has costs[b] = +inf and exactly zero gradient contributions; the other utterances of the batch are unaffected.  A
 * NaN cost from non-finite inputs stays NaN.  Nothing synchronises; the frames are not validated on the device.
 */
int rnnt_engine_loss_fwd_bwd_restrict(const void *logits, const int32_t *targets,
                                      const int32_t *logit_lens, const int32_t *target_lens, int B,
                                      int T, int U1, int V, int blank, float clamp,
                                      float fastemit_lambda, float delay_penalty,
                                      const int32_t *restrict_frames, int restrict_left,
                                      int restrict_right, int dtype, float *costs, void *grad_logits,
                                      void *workspace, size_t ws_bytes, void *stream);
int rnnt_engine_joint_loss_fwd_bwd_restrict(const void *enc, const int64_t enc_strides[3],
                                            const void *pred, const void *W, const void *bias,
                                            const int32_t *targets, const int32_t *logit_lens,
                                            const int32_t *target_lens, int B, int T, int U1, int H,
                                            int V, int blank, float clamp, float grad_scale,
                                            float fastemit_lambda, float delay_penalty,
                                            const int32_t *restrict_frames, int restrict_left,
                                            int restrict_right, int dtype, float *costs, void *grad_enc,
                                            void *grad_pred, void *grad_W, void *grad_bias,
                                            void *workspace, size_t ws_bytes, void *stream);
int rnnt_engine_joint_loss_fwd_restrict(const void *enc, const int64_t enc_strides[3], const void *pred,
                                        const void *W, const void *bias, const int32_t *targets,
                                        const int32_t *logit_lens, const int32_t *target_lens, int B,
                                        int T, int U1, int H, int V, int blank, float delay_penalty,
                                        const int32_t *restrict_frames, int restrict_left,
                                        int restrict_right, int dtype, float *costs, void *workspace,
                                        size_t ws_bytes, void *stream);

/*
 * Forced alignment: the best path through the same lattice, with the same log-probs
 * (lp_blank, lp_emit) as the loss, padded H / V of each route included.  For utterance b with
 * T_b = logit_lens[b], U_b = target_lens[b], a path runs from (0,0) to (T_b-1, U_b): a label arc
 * (t,u) -> (t,u+1) adds lp_emit(t,u) (the log-prob of targets[b,u]), a blank arc (t,u) -> (t+1,u)
 * adds lp_blank(t,u), and the final blank out of (T_b-1, U_b) ends it.
 *   scores [B] fp32 out: log-probability of the best path (accumulated in fp64);
 *   frames [B, U1-1] int32 out: frames[b,u] = the frame at which label u is emitted (non-decreasing, in
 *          [0, T_b-1]) for u < U_b, -1 for u >= U_b.
 * Ties: where the two predecessors of a cell score exactly equal, the path takes the blank
 * predecessor (t-1,u) — with all log-probs equal every label is emitted at frame 0.  A NaN log-prob
 * on any cell the sweep reads makes scores[b] NaN and every frames[b,:] -1; other utterances are
 * unaffected.  No state carries over between calls; the workspace needs no initialisation; results
 * are bit-identical from run to run.  Neither entry needs more workspace than the loss entry of the
 * same shape, so a caller's loss workspace serves both.
 */
/* best alignment on given logits [B,T,U1,V] fp32; workspace <= rnnt_engine_loss_workspace_bytes(B,T,U1,V,RNNT_DTYPE_F32) */
int rnnt_engine_align(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                      const int32_t *target_lens, int B, int T, int U1, int V, int blank,
                      float *scores, int32_t *frames, void *workspace, size_t ws_bytes, void *stream);
/* fused joint + best alignment, every dtype of the fused entry; workspace <= rnnt_engine_workspace_bytes(...) */
int rnnt_engine_joint_align(const void *enc, const int64_t enc_strides[3], const void *pred,
                            const void *W, const void *bias, const int32_t *targets,
                            const int32_t *logit_lens, const int32_t *target_lens, int B, int T,
                            int U1, int H, int V, int blank, int dtype, float *scores,
                            int32_t *frames, void *workspace, size_t ws_bytes, void *stream);

/*
 * CTC auxiliary head: the CTC loss of a Linear(H, V) head on the encoder output — the companion of the
 * transducer loss in hybrid training, (1 - w) rnnt + w ctc — and the frame-wise greedy decode of the same logits.  The reference
 * has neither; the semantics are torch.nn.functional.ctc_loss's on log_softmax(logits) with reduction "none".  Feature test: the
 * symbols below (the ABI version stays 4).
 *   logits [N,T,V] fp32 contiguous, V % 4 == 0 (log-softmax is fused); targets [N,U] int32 (U >= 0; entries at u >= target_lens[n]
 *   are never read; an entry outside [0,V) is read as the nearest valid one); logit_lens / target_lens [N] int32, clamped by the
 *   kernels into 1 .. T and 0 .. U; blank any index in [0,V); U <= 1023 (two lattice states per lane of a 1024-thread workgroup).
 * rnnt_engine_ctc_loss_fwd_bwd:
 *   costs [N] out: -log P(targets | logits) over the T_n x (2 U_n + 1) lattice (fp64 sums).  An utterance without a valid path
 *       (T_n < U_n + its adjacent equal labels) has cost +inf; a NaN logit in a frame t < T_n makes that utterance's cost NaN;
 *       the others are unaffected either way.  U_n = 0 is the one-state lattice of all-blank frames.
 *   grad [N,T,V] out, or NULL (costs only): cost_weights[n] d costs[n] / d logits (cost_weights NULL: 1).  Frames t >= T_n, every
 *       frame of an utterance whose cost is +inf and every frame of an utterance whose weight is 0 get exact zeros.  No atomics:
 *       the occupancies of a repeated label are summed in a fixed order, two calls on the same inputs give the same bits.
 *   ws: scratch of rnnt_engine_ctc_workspace_bytes(N, T, U, V) bytes, 256-byte aligned, no initialisation needed.
 * rnnt_engine_ctc_greedy_decode: per frame t < T_n the argmax (lowest index on ties), then per utterance frames equal to their
 *   predecessor and blanks are dropped: tokens[n, 0 .. counts[n]-1] are the labels in order (tokens [N,T] int32, the rest of a
 *   row is scratch), counts [N].  Two launches for the whole batch, no workspace.
 * Both only enqueue.  Checked before anything is enqueued: RNNT_ERR_INVALID_ARG (null or misaligned pointers, non-positive N, T
 * or V, negative U, blank outside [0,V)), RNNT_ERR_UNSUPPORTED (U > 1023, V % 4 != 0), RNNT_ERR_WORKSPACE.
 */
int rnnt_engine_ctc_workspace_bytes(int N, int T, int U, int V, size_t *out);
int rnnt_engine_ctc_loss_fwd_bwd(const void *logits, const int32_t *targets, const int32_t *logit_lens,
                                 const int32_t *target_lens, int N, int T, int U, int V, int blank,
                                 const float *cost_weights /* [N] or NULL = 1 */, float *costs /* [N] */,
                                 float *grad /* [N,T,V] or NULL: forward only */, void *ws, size_t ws_bytes, void *stream);
int rnnt_engine_ctc_greedy_decode(const void *logits, const int32_t *logit_lens, int N, int T, int V, int blank,
                                  int32_t *tokens /* [N,T] */, int32_t *counts /* [N] */, void *stream);

/*
 * Backward of the UNFUSED joint: given d loss / d logits (any upstream gradient, [B,T,U1,V]
 * contiguous fp32) returns the gradients autograd sends through reference rnnt/joint.py:32-39
 * (joint_ln, tanh, the broadcast add): grad_enc [B,T,H], grad_pred [B,U1,H], grad_W [V,H],
 * grad_bias [V].  Serves callers that keep `joint(...)` and the loss as two calls (a maintainer
 * who swaps only rnnt/joint.py); fp32 only.
 */
int rnnt_engine_joint_bwd_workspace_bytes(int B, int T, int U1, int H, int V, int dtype, size_t *out);
int rnnt_engine_joint_bwd(const void *enc, const int64_t enc_strides[3], const void *pred,
                          const void *W, const void *grad_logits, int B, int T, int U1, int H, int V,
                          int dtype, void *grad_enc, void *grad_pred, void *grad_W, void *grad_bias,
                          void *workspace, size_t ws_bytes, void *stream);

/*
 * Greedy-decode scan (next-step row SURVEY.md 8f-2).  The reference's decode loop, rnnt/model.py:108-125,
 * evaluates joint.single_forward (rnnt/joint.py:44-55) for one audio frame at a time and syncs on
 * argmax(...).item() per frame.  This call evaluates frames t0 .. t0+nframes-1 (nframes <= 128) of
 * one utterance against ONE predictor state and reduces on the device:
 *   out[0] = first frame whose argmax is not `blank` (t0+nframes if every frame says blank)
 *   out[1] = that token (blank if none);   out[2+k] = argmax of frame t0+k (first index on ties)
 *   enc  [T,H] rows enc_stride_t apart, elements enc_stride_h apart (the permuted encoder view
 *        of rnnt/model.py:102 works), already projected by audio_ln when the model has one;
 *   pred [H] predictor output (after text_ln when present); W [V,H]; bias [V]; out int32[2+nframes].
 */
int rnnt_engine_greedy_scan_workspace_bytes(int nframes, int H, int V, size_t *out);
int rnnt_engine_greedy_scan(const void *enc, int64_t enc_stride_t, int64_t enc_stride_h,
                            const void *pred, const void *W, const void *bias, int t0, int nframes,
                            int H, int V, int blank, int32_t *out, void *workspace, size_t ws_bytes,
                            void *stream);

/*
 * Gradient-norm clip + AdamW step over a list of fp32 tensors (next-step row SURVEY.md 8f-4): what
 * follows loss.backward() in the reference's loop,
 *     total_norm = torch.nn.utils.clip_grad_norm_(params, clip)        rnnt/train.py:136
 *     optimizer.step()            torch.optim.AdamW(lr, betas, eps, weight_decay)   rnnt/train.py:164,
 *                                 rnnt/config/basic_sp_convjs_fullcausal.yaml:82-87
 * as multi-tensor kernels (pointer lists are HOST arrays of DEVICE pointers, packed into kernel
 * arguments; up to 40 tensors per launch).
 *   rnnt_engine_grad_norm   total_norm[0] (device) = 2-norm of all gradients, reduced in a fixed
 *                           order; workspace from rnnt_engine_grad_norm_workspace_bytes.
 *   rnnt_engine_adamw_step  decoupled weight decay, no amsgrad: p *= 1 - lr*wd; m += (1-b1)(g-m);
 *                           v = b2 v + (1-b2) g^2; p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps).
 *                           The hyper-parameters are doubles: their scalar arithmetic (1-b1, 1-b2,
 *                           1-lr*wd, the bias corrections) is done in double, as torch does with python
 *                           floats.  `step` = the update count including this one (>= 1).  When `total_norm`
 *                           (device scalar) is non-NULL and max_norm > 0, every gradient is first
 *                           scaled by min(1, max_norm / (total_norm + 1e-6)) — clip_grad_norm_'s
 *                           coefficient, read on the device: no host synchronisation between
 *                           backward and step; write_clipped_grads != 0 also stores the scaled
 *                           gradients (clip_grad_norm_ works in place).
 *   rnnt_engine_adamw_step_dev  the same update with the step count and the learning rate RESIDENT ON THE
 *                           DEVICE: `step_dev` (int64, the count of updates done so far) is incremented
 *                           by the call, `lr_dev` (float) is read when the kernels run, the three derived
 *                           scalars go through `hyper_dev` (float[4], scratch).  Nothing of the update is
 *                           baked into the launch arguments, so the call can be captured into a HIP graph
 *                           and replayed every iteration (an LR scheduler writes lr_dev between replays).
 * The first moment follows Tensor.lerp_: m + (1-b1)(g-m) while 1-b1 < 0.5, g - (g-m) b1 from there (b1 = 0: m = g exactly).
 * Every entry of a list (element count >= 0; a tensor of numel > 0 non-NULL and 4-byte aligned) is checked before the first
 * launch: a refused call (RNNT_ERR_INVALID_ARG) has changed no tensor and not moved `step_dev`.
 */
int rnnt_engine_grad_norm_workspace_bytes(int n_tensors, const int64_t *numels, size_t *out);
int rnnt_engine_grad_norm(int n_tensors, const void *const *grads, const int64_t *numels,
                          float *total_norm, void *workspace, size_t ws_bytes, void *stream);
int rnnt_engine_adamw_step(int n_tensors, void *const *params, const void *const *grads,
                           void *const *exp_avg, void *const *exp_avg_sq, const int64_t *numels,
                           double lr, double beta1, double beta2, double eps, double weight_decay,
                           int64_t step, const float *total_norm, float max_norm,
                           int write_clipped_grads, void *stream);
int rnnt_engine_adamw_step_dev(int n_tensors, void *const *params, const void *const *grads,
                               void *const *exp_avg, void *const *exp_avg_sq, const int64_t *numels,
                               const float *lr_dev, double beta1, double beta2, double eps,
                               double weight_decay, int64_t *step_dev, float *hyper_dev,
                               const float *total_norm, float max_norm, int write_clipped_grads,
                               void *stream);

/*
 * ConvPredictor forward / backward (next-step row SURVEY.md 8f-3): reference rnnt/predictor.py:189-229
 * — embedding, LayerNorm, CausalConv1d k=3 + GELU + dropout, CausalConv1d k=5 + GELU + dropout
 * (rnnt/causalconv.py:9-32: left zero padding), Linear, LayerNorm — on rows (b,u) with channels
 * contiguous: the two permutes of predictor.py:216,225 are never materialised, each convolution is
 * one MFMA GEMM per tap.  All pointers fp32 device pointers, 16-byte aligned; E % 4 == 0, O % 4 == 0.
 *   ids [B,U1] int64 (as the reference passes them, rnnt/model.py:20-21); out [B,U1,O];
 *   keep1 / keep2 [B,U1,E] bytes: dropout keep masks drawn by the caller (NULL = eval mode), kept
 *   values are scaled by 1/(1-dropout_p);  ln_in_eps / ln_out_eps: the eps of input_layer_norm / output_layer_norm
 *   (torch.nn.LayerNorm's default: 1e-5 each);
 *   `saved`: caller-owned buffer (rnnt_engine_conv_predictor_saved_bytes) the forward fills and the
 *   backward of the SAME call reads; `g`: where each parameter's gradient is written (same field
 *   order as the parameters; every gradient is overwritten, not accumulated).
 */
typedef struct rnnt_conv_predictor_params {
    const float *embedding;           /* [S,E]                 embedding.weight           */
    const float *ln_in_w, *ln_in_b;   /* [E]                   input_layer_norm.*         */
    const float *conv1_w, *conv1_b;   /* [E,E,3], [E]          conv1.conv.* (Conv1d layout) */
    const float *conv2_w, *conv2_b;   /* [E,E,5], [E]          conv2.conv.*               */
    const float *linear_w, *linear_b; /* [O,E], [O]            linear.*                   */
    const float *ln_out_w, *ln_out_b; /* [O]                   output_layer_norm.*        */
} rnnt_conv_predictor_params;

int rnnt_engine_conv_predictor_saved_bytes(int B, int U1, int S, int E, int O, size_t *out);
int rnnt_engine_conv_predictor_fwd(const int64_t *ids, int B, int U1, int S, int E, int O,
                                   const rnnt_conv_predictor_params *p, const uint8_t *keep1,
                                   const uint8_t *keep2, float dropout_p, float ln_in_eps, float ln_out_eps, float *out,
                                   void *saved, size_t saved_bytes, void *stream);
int rnnt_engine_conv_predictor_bwd(const int64_t *ids, int B, int U1, int S, int E, int O,
                                   const rnnt_conv_predictor_params *p, const uint8_t *keep1,
                                   const uint8_t *keep2, float dropout_p, const float *grad_out,
                                   const rnnt_conv_predictor_params *g, void *saved, size_t saved_bytes,
                                   void *stream);

/*
 * LSTMPredictor forward / backward / stateful step: reference rnnt/predictor.py:11-186 — embedding, LayerNorm,
 * L layer-normalised LSTM layers (gates = x2g(x_t) + p2g(h_{t-1}), g_norm over all 4 Hd gates of a row, gate order input /
 * forget / cell / output, c = c_norm(f c + i g) — the NORMALISED cell continues —, h = o tanh(c)), dropout after every layer, Linear,
 * LayerNorm — on rows (b,u).  Exact fp32 products.  All pointers fp32 device pointers, 16-byte aligned, except `p->layers` / `g->layers`:
 * HOST arrays of L structs.  Feature test: the symbols below (the ABI version stays 4).
 *   ids [B,U1] int64; out [B,U1,O]; S symbols, E embedding width (layer 0's input), Hd hidden width, O output width;
 *   layer_norm != 0: g_norm / c_norm present and x2g has no bias (x2g_b NULL); 0: no norms (their pointers NULL), x2g_b present;
 *   state_in / state_out [L][2][B][Hd] (h then c of each layer); state_in NULL = zeros; state_out = the state after step U1-1 (h before
 *   dropout); every row runs all U1 steps.  U1 = 1 with a state is the decode step.
 *   keep [L][B,U1,Hd] bytes: dropout keep masks drawn by the caller (NULL = eval mode), kept values x 1/(1-dropout_p);
 *   eps_in / eps_lstm / eps_out: input_layer_norm's, the LSTM layers' and output_layer_norm's eps;
 *   `saved` (rnnt_engine_lstm_predictor_saved_bytes): what the backward of the SAME call reads; NULL = inference, nothing is kept;
 *   `ws` (rnnt_engine_lstm_predictor_workspace_bytes, backward = 0 for _fwd, 1 for _bwd): scratch, free after the call's work ran;
 *   `g`: where each parameter's gradient is written (the parameters' field order; overwritten, not accumulated).  There is no
 *   gradient through the state.
 * Two launches per time step and layer (the recurrent GEMM and one row kernel), no workgroup waits on another; no atomics, every
 * reduction in a fixed order: results are bitwise reproducible.  Every argument is checked before anything is enqueued:
 * RNNT_ERR_INVALID_ARG (null pointers, non-positive dims, dropout_p outside [0,1)), RNNT_ERR_UNSUPPORTED (E % 4, Hd % 4 or O % 4
 * non-zero, Hd > 1024, E > 2048, L > 8), RNNT_ERR_WORKSPACE (short saved / ws).
 */
typedef struct rnnt_lstm_layer_params {
    const float *x2g_w;               /* [4Hd,in]  lstm_layers.l.x2g.weight (in = E for layer 0, else Hd) */
    const float *x2g_b;               /* [4Hd]     lstm_layers.l.x2g.bias; NULL with layer norm           */
    const float *p2g_w;               /* [4Hd,Hd]  lstm_layers.l.p2g.weight                               */
    const float *g_norm_w, *g_norm_b; /* [4Hd]     lstm_layers.l.g_norm.*; NULL without layer norm        */
    const float *c_norm_w, *c_norm_b; /* [Hd]      lstm_layers.l.c_norm.*; NULL without layer norm        */
} rnnt_lstm_layer_params;
typedef struct rnnt_lstm_predictor_params {
    const float *embedding;               /* [S,E]       embedding.weight      */
    const float *ln_in_w, *ln_in_b;       /* [E]         input_layer_norm.*    */
    const float *linear_w, *linear_b;     /* [O,Hd], [O] linear.*              */
    const float *ln_out_w, *ln_out_b;     /* [O]         output_layer_norm.*   */
    const rnnt_lstm_layer_params *layers; /* host array of L                   */
} rnnt_lstm_predictor_params;

int rnnt_engine_lstm_predictor_saved_bytes(int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm, size_t *out);
int rnnt_engine_lstm_predictor_workspace_bytes(int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm, int backward,
                                               size_t *out);
int rnnt_engine_lstm_predictor_fwd(const int64_t *ids, int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm,
                                   const rnnt_lstm_predictor_params *p, const float *state_in, const uint8_t *keep,
                                   float dropout_p, float eps_in, float eps_lstm, float eps_out, float *out, float *state_out,
                                   void *saved, size_t saved_bytes, void *ws, size_t ws_bytes, void *stream);
int rnnt_engine_lstm_predictor_bwd(const int64_t *ids, int B, int U1, int S, int E, int Hd, int O, int L, int layer_norm,
                                   const rnnt_lstm_predictor_params *p, const uint8_t *keep, float dropout_p, float eps_in,
                                   float eps_lstm, float eps_out, const float *d_out, const rnnt_lstm_predictor_params *g,
                                   const void *saved, size_t saved_bytes, void *ws, size_t ws_bytes, void *stream);

/*
 * Device-resident greedy decode of ONE utterance (next-step row SURVEY.md 8f-2, second half): the whole loop of
 * rnnt/model.py:108-125 — scan frames from t for the first non-blank argmax, append the token, at most `max_per_frame`
 * tokens per frame, re-run the predictor — with the stateless ConvPredictor of rnnt/predictor.py:189-229 (eval mode:
 * no dropout) evaluated incrementally on the device (its output frame is a function of the last 7 tokens).  The call
 * only ENQUEUES: (init != 0) state initialisation, then `iterations` times a fixed kernel sequence (0 = the upper bound
 * max_length + ceil(T / scan_frames) + 1) whose kernels return at once after the loop has ended.  A caller may enqueue the
 * bound in one call, or a chunk at a time (init = 1 first, then init = 0 with the same buffers) and stop when the loop is
 * over: `host_flag` (NULL, or one int32 of PINNED host memory the caller zeroed) is set to 1 by the device when the loop
 * ends and can be polled without a synchronisation.  The caller synchronises once and reads
 *   state  int32[RNNT_DECODE_STATE_WORDS]: [RNNT_DECODE_T] t, [RNNT_DECODE_EMITTED] emitted, [RNNT_DECODE_NTOK] ntok = decoded tokens,
 *          [RNNT_DECODE_DONE] done, [RNNT_DECODE_NEWTOK] a label the predictor has still to take in, [RNNT_DECODE_ITERATIONS]
 *          iterations that did work; word 6 is [RNNT_DECODE_SETTLED] in rnnt_engine_greedy_decode_lstm's state and
 *          [RNNT_DECODE_WORKGROUPS] in rnnt_engine_greedy_decode_persistent's, which also sets [RNNT_DECODE_CODE];
 *   tokens int32[max_length]: tokens[0] = blank (rnnt/model.py:100), tokens[1 .. ntok] = the decoded ids.
 * frames [T,H] fp32 audio frames, rows frame_stride apart, unit element stride (already projected by audio_ln when the
 * joint has one); text_W [H,O] / text_b [H]: joint.text_ln, or NULL when the joint adds the predictor output directly
 * (then O == H); W [V,H], bias [V]: joint_ln.  E, O <= 1024, E % 4 == 0, O % 4 == 0, H % 8 == 0, V % 4 == 0,
 * 1 <= scan_frames <= 128, max_length >= 2.
 */
#define RNNT_DECODE_STATE_WORDS 8
#define RNNT_DECODE_T 0
#define RNNT_DECODE_EMITTED 1
#define RNNT_DECODE_NTOK 2
#define RNNT_DECODE_DONE 3
#define RNNT_DECODE_NEWTOK 4
#define RNNT_DECODE_ITERATIONS 5
#define RNNT_DECODE_SETTLED 6     /* rnnt_engine_greedy_decode_lstm */
#define RNNT_DECODE_WORKGROUPS 6  /* rnnt_engine_greedy_decode_persistent */
#define RNNT_DECODE_CODE 7        /* rnnt_engine_greedy_decode_persistent: != 0 = not a decode */
int rnnt_engine_greedy_decode_workspace_bytes(int H, int V, int E, int O, int scan_frames, size_t *out);
int rnnt_engine_greedy_decode(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                              int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                              const void *W, const void *bias, int H, int V, int blank, int max_length,
                              int max_per_frame, int scan_frames, int iterations, int init, int32_t *host_flag,
                              int32_t *state, int32_t *tokens, void *workspace, size_t ws_bytes, void *stream);

/*
 * The same loop with the stateful LSTMPredictor (rnnt/predictor.py:93-186, eval mode; DESIGN.md 4p "Device decode") for n_utt
 * (1 .. 32) INDEPENDENT utterances advancing in lockstep: the rows of one 32-row tile of every product.  Per iteration a fixed
 * kernel sequence: embedding + input LayerNorm of the utterances that emitted a label, per layer both gate products in one launch
 * and one row step (h and c updated in place; a row whose utterance emitted nothing keeps its h, c and text vector), linear + output
 * LayerNorm, joint.text_ln where the joint has one, the scan of `scan_frames` frames from each utterance's own t (tanh of the sum: no
 * range limit), argmax + bookkeeping per utterance.  5 + 2 L launches per iteration, 2 more with text_ln.
 *   frames: `rows` packed rows [rows,H], frame_stride apart; utt: DEVICE int32[n_utt][2] = each utterance's first row and frame count
 *   (the convention of rnnt_engine_beam_decode_batch; the kernels hold every entry inside the buffer); max_frames: the longest count.
 *   p, S, E, Hd, O, L, layer_norm, eps_in / eps_lstm / eps_out: as rnnt_engine_lstm_predictor_fwd; text_W .. max_per_frame, scan_frames,
 *   iterations (0 = the bound max_length + ceil(max_frames / scan_frames) + 1), init, host_flag (raised when ALL utterances have
 *   ended): as rnnt_engine_greedy_decode.
 *   state  int32[n_utt][RNNT_DECODE_STATE_WORDS]: the words of rnnt_engine_greedy_decode's, [RNNT_DECODE_SETTLED] settled (done, and the
 *   last label taken in); tokens int32[n_utt][max_length]: row u as rnnt_engine_greedy_decode's.
 *   state_out: NULL or [L][2][n_utt][Hd], the LSTM state after each utterance's last label (after the start blank if it has none).
 *   The workspace BEGINS with the text vectors [n_utt][H] (the joint's text input after each utterance's last label).
 * An utterance's tokens, state words and state_out rows are bit-identical whatever its neighbours, its position and n_utt.
 * Checked before anything is enqueued: RNNT_ERR_INVALID_ARG (null pointers, non-positive dims, max_length < 2), RNNT_ERR_UNSUPPORTED
 * (rnnt_engine_lstm_predictor_fwd's limits, H % 8, V % 4, scan_frames outside 1..128, n_utt > 32), RNNT_ERR_WORKSPACE.
 */
int rnnt_engine_greedy_decode_lstm_workspace_bytes(int n_utt, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V, int has_text,
                                                   int scan_frames, size_t *out);
int rnnt_engine_greedy_decode_lstm(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                   const rnnt_lstm_predictor_params *p, int S, int E, int Hd, int O, int L, int layer_norm, float eps_in,
                                   float eps_lstm, float eps_out, const void *text_W, const void *text_b, const void *W, const void *bias,
                                   int H, int V, int blank, int max_length, int max_per_frame, int scan_frames, int iterations, int init,
                                   int32_t *host_flag, int32_t *state, int32_t *tokens, float *state_out, void *workspace, size_t ws_bytes,
                                   void *stream);

/*
 * Streaming form of rnnt_engine_greedy_decode_lstm (DESIGN.md 4p "Device stream"): n_streams (1 .. 32) INDEPENDENT streams of one model,
 * each decoded push by push, all advancing in lockstep through the same kernel sequence per iteration (5 + 2 L launches, 2 more with
 * text_ln).  After any sequence of pushes that delivered frames 0 .. k-1 of a stream, in any chunking, its labels, its LSTM state and its
 * text vector are bit for bit what rnnt_engine_greedy_decode_lstm gives for those k frames alone with the same max_length and
 * max_per_frame, whatever scan_frames is, whatever the other streams do, whatever n_streams and the stream's slot.
 * Everything a stream carries from push to push lives in the caller's BLOCK (rnnt_engine_greedy_stream_lstm_bytes bytes, 256-byte
 * aligned), three sections each a multiple of 256 bytes:
 *   state  int32[n_streams][RNNT_LSTM_STREAM_STATE_WORDS]:
 *          [RNNT_LSTM_STREAM_T] frames of the CURRENT push consumed, [RNNT_LSTM_STREAM_EMITTED] labels emitted at the current frame,
 *          [RNNT_LSTM_STREAM_LABELS] labels so far over all pushes, [RNNT_LSTM_STREAM_PAUSED] nothing to scan (the push's frames are
 *          consumed, or done), [RNNT_LSTM_STREAM_NEWTOK] the predictor has still to take the newest token in,
 *          [RNNT_LSTM_STREAM_PUSH_ITERATIONS] iterations of this push that did work, [RNNT_LSTM_STREAM_AT_REST] at rest,
 *          [RNNT_LSTM_STREAM_DONE] 1 + labels reached max_length (later pushes consume nothing), [RNNT_LSTM_STREAM_FRAMES] frames
 *          consumed over all pushes, [RNNT_LSTM_STREAM_NEWEST] the newest token (the blank after init), [RNNT_LSTM_STREAM_PUSH_LABELS]
 *          labels this push emitted, [RNNT_LSTM_STREAM_BASE] the frames consumed when the current push began; the others 0;
 *   h, c   float[L][2][n_streams][Hd]: the LSTM state after the stream's last label taken in;
 *   text   float[n_streams][H]: the joint's text input after it.
 * The workspace (rnnt_engine_greedy_stream_lstm_push_workspace_bytes) is scratch only: a push gives the same bits whatever it held.
 * rnnt_engine_greedy_stream_lstm_init starts all streams (index = -1) or stream `index` alone ("this slot starts a new utterance"; no
 * byte of another stream's part of the block is touched) by one kernel: zero LSTM state, newest token = blank, to be taken in, at rest.
 * The step from zero state on the start blank runs in the first push that brings the stream a frame.
 * rnnt_engine_greedy_stream_lstm_push enqueues one push: `frames` holds the push's frames of all streams packed into `rows` >= 1 rows,
 *   push_table device int32[n_streams][2]: stream u's first row and frame count; a count <= 0: the stream sits the push out and no bit of
 *          its words, h, c and text vector changes.  The kernels hold every entry inside the buffer;
 *   max_count: the largest count (>= 0);
 *   begin != 0 opens the push with a kernel that latches each stream's base, clears the at-rest word of the streams that got frames
 *          (and are not done), resets their per-push words and counts the others; begin = 0 continues it (chunked enqueueing);
 *   a stream comes to REST when all its pushed frames are consumed AND no label awaits the predictor: a push that ends on a label
 *          capped by max_per_frame still takes that label in first (the offline loop's "settled");
 *   max_length: 0 = unbounded, else >= 2 as rnnt_engine_greedy_decode_lstm's;
 *   out_tokens int32[n_streams][out_stride]: row u = the labels this push gave stream u, [RNNT_LSTM_STREAM_PUSH_LABELS] of them;
 *          out_stride >= max_count * max_per_frame is required (a stream emits at most that many in a push);
 *   iterations: 0 = the push's bound max_count * max_per_frame + ceil(max_count / scan_frames) + 1 — every iteration of a stream not at
 *          rest emits a label, or consumes a block of scan_frames frames or the rest of the push, and one more takes the last label
 *          in; the pending start step shares the first iteration with its scan and adds none.  The bound does not grow with the
 *          stream's history;
 *   host_flag rises once ALL streams are at rest (a done stream is at rest once its last label is taken in).
 * The model arguments as rnnt_engine_greedy_decode_lstm.  The caller synchronises once per push.  Every argument is checked before
 * anything is enqueued: RNNT_ERR_INVALID_ARG (null or misaligned pointers, non-positive dims, max_length 1 or negative, negative
 * max_count, rows < 1, index outside -1 .. n_streams - 1, out_stride too small), RNNT_ERR_UNSUPPORTED (n_streams > 32, scan_frames
 * outside 1..128, rnnt_engine_lstm_predictor_fwd's limits, H % 8, V % 4), RNNT_ERR_WORKSPACE (a short workspace or a short block).
 * The model's weights must not change while a stream is open.
 */
#define RNNT_LSTM_STREAM_STATE_WORDS 16
#define RNNT_LSTM_STREAM_T 0
#define RNNT_LSTM_STREAM_EMITTED 1
#define RNNT_LSTM_STREAM_LABELS 2
#define RNNT_LSTM_STREAM_PAUSED 3
#define RNNT_LSTM_STREAM_NEWTOK 4
#define RNNT_LSTM_STREAM_PUSH_ITERATIONS 5
#define RNNT_LSTM_STREAM_AT_REST 6
#define RNNT_LSTM_STREAM_DONE 7
#define RNNT_LSTM_STREAM_FRAMES 8
#define RNNT_LSTM_STREAM_NEWEST 9
#define RNNT_LSTM_STREAM_PUSH_LABELS 10
#define RNNT_LSTM_STREAM_BASE 11
int rnnt_engine_greedy_stream_lstm_bytes(int n_streams, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V, int has_text,
                                         size_t *out);
int rnnt_engine_greedy_stream_lstm_init(int n_streams, int Hd, int L, int H, int blank, int index, void *block, size_t bytes, void *stream);
int rnnt_engine_greedy_stream_lstm_push_workspace_bytes(int n_streams, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V,
                                                        int has_text, int scan_frames, size_t *out);
int rnnt_engine_greedy_stream_lstm_push(const void *frames, int64_t frame_stride, int rows, const int32_t *push_table, int n_streams,
                                        int max_count, const rnnt_lstm_predictor_params *p, int S, int E, int Hd, int O, int L,
                                        int layer_norm, float eps_in, float eps_lstm, float eps_out, const void *text_W,
                                        const void *text_b, const void *W, const void *bias, int H, int V, int blank, int max_length,
                                        int max_per_frame, int scan_frames, int iterations, int begin, int32_t *host_flag,
                                        int32_t *out_tokens, int out_stride, void *block, size_t bytes, void *workspace, size_t ws_bytes,
                                        void *stream);

/*
 * The same loop (rnnt/model.py:108-125 with the ConvPredictor of rnnt/predictor.py:189-229, eval mode) for one utterance as ONE
 * persistent launch: 16 - 128 workgroups stay resident for the whole utterance and hand scan candidates, the conv2 output and the
 * predictor's output to each other through tagged 8-byte words in the workspace (rnnt_amd/csrc/decode.hip, k_dec_persist), with
 * conv1 replaced by per-token table rows and joint.text_ln folded into the predictor's linear layer (tables and folded matrices
 * come from `tables`, below: the caller's buffer, or rebuilt from the parameters inside this call).  Same arguments, state and tokens
 * as rnnt_engine_greedy_decode without scan_frames / iterations / init (the block is 16 frames, the call is the whole decode);
 * state[RNNT_DECODE_ITERATIONS] = iterations, state[RNNT_DECODE_WORKGROUPS] = workgroups, state[RNNT_DECODE_CODE] != 0: the loop did NOT decode (state and tokens are then not a decode;
 * nothing is raised on the stream) — 1..9: a hand-off never arrived within the bounded spin (~0.4 s: a workgroup was not resident)
 * and the loop gave up; 10 / 11: an audio frame / a text vector holds an entry beyond +-30 or a non-finite one, where the loop's
 * factored tanh(e + p) = 1 - 2 / (1 + exp 2e exp 2p) is not exact.  In every such case decode the utterance with
 * rnnt_engine_greedy_decode, which needs no residency and takes tanh of the sum.  The call only enqueues; the caller synchronises once.
 * RNNT_ERR_UNSUPPORTED (call rnnt_engine_greedy_decode instead): H % 64 != 0, H / E / O > 1024, S > 4096, T + max_length >= 2^20,
 * a device with fewer compute units than workgroups or with less LDS per workgroup than the kernel keeps (100-138 KB).  Token lists
 * equal rnnt_engine_greedy_decode's wherever the argmax is not a rounding-level tie (sums are associated differently).
 */
int rnnt_engine_greedy_decode_persistent_workspace_bytes(int T, int S, int E, int O, int H, int V, int has_text, size_t *out);
/* `tables`: NULL (the tables are rebuilt in the workspace by this call: ~0.13 ms) or a caller-owned buffer filled by
 * rnnt_engine_greedy_decode_build_tables for the SAME parameters (conv2's pack, the conv1 tap tables, the folded text_ln): build once per
 * set of weights, decode any number of utterances — concurrently on several streams too (the tables are only read).  The tables take
 * any S (the beam searches bring them too); S > 4096 is refused by the persistent loop's own size query, not here. */
int rnnt_engine_greedy_decode_tables_bytes(int S, int E, int O, int H, int has_text, size_t *out);
int rnnt_engine_greedy_decode_build_tables(const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, const void *text_W,
                                           const void *text_b, int H, void *tables, size_t tables_bytes, void *stream);
int rnnt_engine_greedy_decode_persistent(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                                         int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                                         const void *W, const void *bias, int H, int V, int blank, int max_length,
                                         int max_per_frame, const void *tables, int32_t *host_flag, int32_t *state, int32_t *tokens,
                                         void *workspace, size_t ws_bytes, void *stream);

/*
 * Streaming greedy decode: the loop of rnnt_engine_greedy_decode carried from one chunk of audio frames (a "push") to
 * the next.  For every way of cutting an utterance's frames into pushes, empty ones included, the labels of the pushes concatenated
 * equal the decode of all frames at once with the same max_length.  The caller owns the stream's state, a device block of
 * RNNT_STREAM_STATE_WORDS int32:
 *   [RNNT_STREAM_FRAMES] frames consumed, [RNNT_STREAM_EMITTED] labels emitted at the current frame, [RNNT_STREAM_LABELS] labels so far,
 *   [RNNT_STREAM_DONE] 1 once 1 + labels reached max_length (later pushes consume nothing),
 *   [RNNT_STREAM_TOKENS + j] j < 7: the last 7 tokens, newest first, the leading blank included, -1 before the start,
 *   [RNNT_STREAM_PUSH_LABELS] labels the last push emitted, [RNNT_STREAM_PUSH_ITERATIONS] its iterations that did work,
 *   [RNNT_STREAM_STATUS] its status: 0, or a persistent push's state[RNNT_DECODE_CODE] of rnnt_engine_greedy_decode_persistent (1..9 a hand-off
 *   never arrived, 10 / 11 an audio frame / a text vector beyond +-30).  A push with a non-zero status changes only the three push
 *   words: redo it from the same state with persistent = 0.
 * rnnt_engine_greedy_stream_init writes the initial block ([blank, -1 x 6] as the tokens, zeros elsewhere) by a kernel.
 * rnnt_engine_greedy_stream_decode enqueues one push of n >= 0 frames (rows frame_stride apart, unit element stride, audio_ln already
 * applied; frame 0 is the push's first) and writes its labels to out_tokens[0 .. state[RNNT_STREAM_PUSH_LABELS]) — room for
 * n * max_per_frame labels, or fewer when max_length leaves fewer.  max_length 0 = unbounded, else >= 2 (labels + 1 <= max_length).
 * Model arguments as rnnt_engine_greedy_decode_persistent; `tables` as there.  persistent = 1: one k_dec_persist launch resumed from the
 * block (RNNT_ERR_UNSUPPORTED where the persistent decode refuses the sizes or n + n * max_per_frame >= 2^20); 0: the kernel-per-layer
 * loop, rings refilled from the last 7 tokens.  Both leave the same labels wherever the argmax is not a rounding-level tie.  The
 * workspace query with persistent = 1 covers both paths.  Every argument is checked before anything is enqueued; the call only
 * enqueues, the caller synchronises once per push.  The model's weights and tables must not change while a stream is open.
 */
#define RNNT_STREAM_STATE_WORDS 16
#define RNNT_STREAM_FRAMES 0
#define RNNT_STREAM_EMITTED 1
#define RNNT_STREAM_LABELS 2
#define RNNT_STREAM_DONE 3
#define RNNT_STREAM_TOKENS 4
#define RNNT_STREAM_PUSH_LABELS 11
#define RNNT_STREAM_PUSH_ITERATIONS 12
#define RNNT_STREAM_STATUS 13
int rnnt_engine_greedy_stream_init(int32_t *state, int blank, void *stream);
int rnnt_engine_greedy_stream_decode_workspace_bytes(int n, int S, int E, int O, int H, int V, int has_text, int max_length,
                                                     int max_per_frame, int persistent, size_t *out);
int rnnt_engine_greedy_stream_decode(const void *frames, int64_t frame_stride, int n, const rnnt_conv_predictor_params *p,
                                     int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                                     const void *W, const void *bias, int H, int V, int blank, int max_length, int max_per_frame,
                                     const void *tables, int persistent, int32_t *state, int32_t *out_tokens, void *workspace,
                                     size_t ws_bytes, void *stream);

/*
 * Frame-synchronous beam search of ONE utterance on the device, with the stateless ConvPredictor of
 * rnnt/predictor.py:189-229 (eval mode) and the joint of rnnt/joint.py:44-55: at most `max_per_frame` labels per frame,
 * hypotheses merged by token sequence (logaddexp of their scores), output capped at max_length - 1 labels; beam 1 is the
 * reference's greedy decode (rnnt/model.py:95-128 with max_per_frame = 10).  The call only ENQUEUES: (init != 0) the search's
 * initialisation, then `iterations` ROUNDS (0 = the upper bound T * max_per_frame + 1), each a fixed kernel sequence whose
 * kernels return at once after the search has ended.  A caller may enqueue the bound in one call, or a chunk at a time
 * (init = 1 first, then init = 0 with the same buffers) and stop when `host_flag` (NULL, or one int32 of PINNED host memory the
 * caller zeroed) has been set to 1 by the device.  The caller synchronises once and reads
 *   state  int32[32]: [0] t, [1] round within the frame, [2] n = entries of the result, [3] done, [5] rounds that did work,
 *                     [8 + j] the length of entry j (labels after the leading blank);
 *   tokens int32[beam, max_length]: tokens[j][0] = blank, tokens[j][1 .. state[8 + j]] the labels of entry j;
 *   scores double[beam]: log-probability of entry j (fp64 accumulation of fp32 log-softmax terms);
 * entries j < n sorted best first.  Arguments as rnnt_engine_greedy_decode; `tables`: NULL (rebuilt in the workspace by every
 * call) or a buffer of rnnt_engine_greedy_decode_build_tables for the SAME parameters.  1 <= beam <= 16 (RNNT_ERR_UNSUPPORTED
 * above), E, O <= 1024, E % 4 == 0, O % 4 == 0, H % 8 == 0, V % 4 == 0, 2 <= max_length <= 65536.  Every argument is checked
 * before anything is enqueued.
 */
int rnnt_engine_beam_decode_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, size_t *out);
int rnnt_engine_beam_decode(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                            int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                            const void *W, const void *bias, int H, int V, int blank, int max_length, int max_per_frame,
                            int beam, const void *tables, int iterations, int init, int32_t *host_flag, int32_t *state,
                            int32_t *tokens, double *scores, void *workspace, size_t ws_bytes, void *stream);

/*
 * The same search for n_utt INDEPENDENT utterances of one model, advanced in lockstep (DESIGN.md §4h "Batched"): every round's
 * kernels carry the utterance as a grid dimension, a search that has ended costs nothing more, and the result of each utterance is
 * bit-identical to rnnt_engine_beam_decode of it alone, whatever its neighbours and its position.  Arguments as
 * rnnt_engine_beam_decode, with
 *   frames: the utterances' frames packed into `rows` rows (frame_stride apart);
 *   utt    device int32[n_utt][2]: utterance u's first row and its frame count T_u >= 1 (rows the table names beyond `rows` are
 *          read as the last row: the caller vouches for `rows`, never for the table);
 *   max_frames: the largest T_u — `iterations` = 0 enqueues the bound max_frames * max_per_frame + 1.  The table lives on the
 *          device, so it is NOT checked against max_frames: an entry above it can leave that search unfinished after the bound
 *          (state[u][3] == 0) — `host_flag` then never rises and the call has still returned RNNT_OK; the caller sees it in
 *          state[u][3] after its synchronisation;
 *   state  int32[n_utt][32], tokens int32[n_utt][beam][max_length], scores double[n_utt][beam]: per utterance as above.
 * beam, max_length, max_per_frame and blank are shared.  `host_flag` is set once ALL searches have ended.  The same iterations /
 * init protocol; the workspace's state part (n_utt times the single search's, and a counter) is zero-filled at init.
 * 1 <= n_utt <= 64 (RNNT_ERR_UNSUPPORTED otherwise, from the query and the call); every other limit as rnnt_engine_beam_decode.
 * Every argument is checked before anything is enqueued.
 */
int rnnt_engine_beam_decode_batch_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, int n_utt,
                                                  size_t *out);
int rnnt_engine_beam_decode_batch(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                  const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, float ln_out_eps,
                                  const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                                  int max_length, int max_per_frame, int beam, const void *tables, int iterations, int init,
                                  int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *workspace, size_t ws_bytes,
                                  void *stream);

/*
 * The same search with the stateful LSTMPredictor (DESIGN.md §4h "LSTM") for n_utt (1 .. 32) independent utterances in lockstep; the
 * single search is n_utt = 1.  predictor([blank] + y)[-1] is the output of ONE step from the state after y[:-1], fed y[-1]; the start
 * is the step from zero state fed the blank.  Row 16 u + s of every product is slot s of utterance u.  A hypothesis owns an LSTM
 * state [L][2][Hd] that lives in one of its utterance's 32 rows of a pool in the workspace and follows it through the selection as
 * an INDEX: a survivor keeps its row, a kept label records its parent's row and takes a row no slot refers to, nothing is copied.
 * A round with a predictor step is 6 + 2 L launches (2 more with text_ln): embedding + input LayerNorm, per layer both gate products
 * (the recurrent operand read through the parent's row) and the row step, linear + output LayerNorm, joint.text_ln, then the joint,
 * reduce and selection kernels of rnnt_engine_beam_decode_batch.  Kernels return at once where no slot awaits a step.
 *   model arguments (p .. eps_out, text_W .. blank) as rnnt_engine_greedy_decode_lstm; frames, rows, utt, max_frames, state
 *   int32[n_utt][32], tokens int32[n_utt][beam][max_length], scores double[n_utt][beam], iterations (0 = max_frames * max_per_frame
 *   + 1), init, host_flag as rnnt_engine_beam_decode_batch.  The workspace's state part (searches, pool) is zero-filled at init; no
 *   value the caller left in the rest is read.
 * An utterance's tokens, state words and scores are bit-identical whatever its neighbours, its position and n_utt.
 * Checked before anything is enqueued: RNNT_ERR_INVALID_ARG (null pointers, non-positive dims, beam < 1, max_length < 2),
 * RNNT_ERR_UNSUPPORTED (n_utt > 32, beam > 16, max_length > 65536, rnnt_engine_lstm_predictor_fwd's limits, H % 8, V % 4),
 * RNNT_ERR_WORKSPACE.
 */
int rnnt_engine_beam_decode_lstm_workspace_bytes(int n_utt, int S, int E, int Hd, int O, int L, int layer_norm, int H, int V, int has_text,
                                                 int max_length, int beam, size_t *out);
int rnnt_engine_beam_decode_lstm(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                 const rnnt_lstm_predictor_params *p, int S, int E, int Hd, int O, int L, int layer_norm, float eps_in,
                                 float eps_lstm, float eps_out, const void *text_W, const void *text_b, const void *W, const void *bias,
                                 int H, int V, int blank, int max_length, int max_per_frame, int beam, int iterations, int init,
                                 int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *workspace, size_t ws_bytes,
                                 void *stream);

/*
 * Contextual biasing (hotword boosting) of the two searches above (DESIGN.md §4h "Context"): rnnt_engine_beam_decode_ctx and
 * rnnt_engine_beam_decode_batch_ctx are rnnt_engine_beam_decode and rnnt_engine_beam_decode_batch with one more argument, a phrase list
 * as an Aho-Corasick trie (ONE graph, shared by every utterance of a batch).  Node 0 is the root; node m's children are entries
 * child_off[m] .. child_off[m + 1] - 1 of child_tok (their tokens, ASCENDING within a node) and child_node (the nodes they lead to);
 * fail_link[m] is the node of the deepest proper suffix of m's path that is a path of the trie (the root's is 0); depth[m] (0 .. 64) the
 * length of m's path, bonus(m) = score * depth[m]; terminal[m] != 0 where a phrase ends.  A hypothesis at node n that takes label k:
 *   m = n; while m != 0 and k is no child of m: m = fail_link[m];  m' = child(m, k) if there is one, else 0;
 *   its score gains delta = score * (depth[m'] - depth[n]);  its node becomes 0 if terminal[m'] (the bonus is banked), else m'.
 * Blank candidates gain nothing.  The scores kept during the search AND RETURNED in `scores` are INTERNAL: they still hold the bonus
 * of an unfinished match.  The caller FINALISES: walk entry j's labels through the graph from node 0 to its node n_j, report
 * scores[j] - score * depth[n_j], and re-sort the entries by that value (stable, descending).
 * The arrays live on the device, so their CONTENTS are not checked: the kernels clamp every node index to [0, n_nodes), every child
 * range to [0, n_children], every depth to [0, 64], walk at most 64 fail links per step and bisect a child range in at most 32 steps — a
 * malformed graph gives a wrong result, never an access out of range or a loop without end.  Refused before anything is enqueued:
 * a null `ctx` or null array, n_nodes < 1, n_children outside [0, n_nodes) (a trie has n_nodes - 1), a negative or non-finite score
 * (RNNT_ERR_INVALID_ARG), n_nodes > 65536 (RNNT_ERR_UNSUPPORTED), and everything the plain entry points refuse.  The workspace holds
 * one node per slot more than the plain search's: each entry point has its own query.  RNNT_ENGINE_VERSION is unchanged: detect the
 * feature by symbol.
 */
#define RNNT_BEAM_CONTEXT_MAX_NODES 65536
typedef struct rnnt_beam_context {
    int32_t n_nodes, n_children;
    double score;
    const int32_t *child_off;  /* device int32[n_nodes + 1] */
    const int32_t *child_tok;  /* device int32[max(n_children, 1)] */
    const int32_t *child_node; /* device int32[max(n_children, 1)] */
    const int32_t *fail_link;  /* device int32[n_nodes] */
    const int32_t *depth;      /* device int32[n_nodes] */
    const int32_t *terminal;   /* device int32[n_nodes] */
} rnnt_beam_context;
int rnnt_engine_beam_decode_ctx_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, size_t *out);
int rnnt_engine_beam_decode_ctx(const void *frames, int64_t frame_stride, int T, const rnnt_conv_predictor_params *p,
                                int S, int E, int O, float ln_in_eps, float ln_out_eps, const void *text_W, const void *text_b,
                                const void *W, const void *bias, int H, int V, int blank, int max_length, int max_per_frame,
                                int beam, const void *tables, int iterations, int init, int32_t *host_flag, int32_t *state,
                                int32_t *tokens, double *scores, void *workspace, size_t ws_bytes, const rnnt_beam_context *ctx,
                                void *stream);
int rnnt_engine_beam_decode_batch_ctx_workspace_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam,
                                                      int n_utt, size_t *out);
int rnnt_engine_beam_decode_batch_ctx(const void *frames, int64_t frame_stride, int rows, const int32_t *utt, int n_utt, int max_frames,
                                      const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, float ln_out_eps,
                                      const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                                      int max_length, int max_per_frame, int beam, const void *tables, int iterations, int init,
                                      int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *workspace,
                                      size_t ws_bytes, const rnnt_beam_context *ctx, void *stream);

/*
 * Streaming beam search: the search of rnnt_engine_beam_decode stopped at frame boundaries, for n_streams (1 .. 64)
 * INDEPENDENT streams of one model advanced in lockstep by the batched search's kernel sequence.  After any sequence of pushes that
 * delivered frames 0 .. k-1 of a stream, in any chunking, its result is bit for bit what rnnt_engine_beam_decode returns for those k
 * frames: a stream that completes the last frame of its push comes to REST (its result is written as at `done`, its kernels return at
 * once) and the next push resumes from that very state.  The search never ends: max_length only stops hypotheses growing.
 * Everything a stream carries from push to push lives in caller-owned memory:
 *   block  rnnt_engine_beam_stream_bytes(...) bytes, 256-byte aligned: per stream the slot buffers and per-round intermediates of the
 *          single search's workspace, and a counter.  A push uses no other scratch; the decode tables
 *          (rnnt_engine_greedy_decode_build_tables) are REQUIRED and shared;
 *   state  int32[n_streams][32]: words 1 .. 6 and 8 .. 23 as rnnt_engine_beam_decode's, [RNNT_BEAM_STREAM_FRAMES] the frames consumed
 *          over all pushes, [3] always 0, [RNNT_BEAM_STREAM_AT_REST] 1 while every frame pushed so far is consumed,
 *          [RNNT_BEAM_STREAM_BASE] the frames consumed when the current push began;
 *   tokens int32[n_streams][beam][max_length], scores double[n_streams][beam]: the result after the last push, as above.
 * rnnt_engine_beam_stream_init starts all streams (index = -1) or stream `index` alone ("this slot starts a new utterance", the others
 * untouched) by kernels: the empty hypothesis, at rest, and the result of zero frames (one entry, length 0, score 0.0).
 * rnnt_engine_beam_stream_push enqueues one push: `frames` holds the push's frames of all streams packed into `rows` >= 1 rows,
 *   push_table device int32[n_streams][2]: stream u's first row in THIS push's frames and its frame count; 0 (or less): the stream
 *          sits the push out.  Frame t of a stream is row first + (t - base), read as the last row beyond `rows`;
 *   max_count: the largest count (>= 0) — `iterations` = 0 enqueues the bound max_count * max_per_frame + 1 rounds;
 *   begin != 0 opens the push with a kernel that latches each stream's base, clears the at-rest word of the streams that got frames
 *          and counts the others; begin = 0 continues it (chunked enqueueing, as `init` of rnnt_engine_beam_decode);
 *   host_flag rises once ALL streams are at rest.
 * The other arguments as rnnt_engine_beam_decode_batch.  The caller synchronises once per push.  Limits as
 * rnnt_engine_beam_decode_batch (RNNT_ERR_UNSUPPORTED: beam > 16, n_streams outside 1 .. 64, sizes the beam kernels refuse;
 * RNNT_ERR_WORKSPACE: a short block; RNNT_ERR_INVALID_ARG: null pointers or table, negative counts); every argument is checked before
 * anything is enqueued.  The model's weights and tables must not change while a stream is open.
 */
#define RNNT_BEAM_STREAM_FRAMES 0
#define RNNT_BEAM_STREAM_AT_REST 24
#define RNNT_BEAM_STREAM_BASE 25
int rnnt_engine_beam_stream_bytes(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, int n_streams, size_t *out);
int rnnt_engine_beam_stream_init(int S, int E, int O, int H, int V, int has_text, int max_length, int beam, int blank, int n_streams,
                                 int index, int32_t *state, double *scores, void *block, size_t bytes, void *stream);
int rnnt_engine_beam_stream_push(const void *frames, int64_t frame_stride, int rows, const int32_t *push_table, int n_streams, int max_count,
                                 const rnnt_conv_predictor_params *p, int S, int E, int O, float ln_in_eps, float ln_out_eps,
                                 const void *text_W, const void *text_b, const void *W, const void *bias, int H, int V, int blank,
                                 int max_length, int max_per_frame, int beam, const void *tables, int iterations, int begin,
                                 int32_t *host_flag, int32_t *state, int32_t *tokens, double *scores, void *block, size_t bytes,
                                 void *stream);

/*
 * y = x W^T + b and its backward as MFMA kernels: the joint's optional input projections
 * audio_ln / text_ln (next-step row SURVEY.md 8f-1; reference rnnt/joint.py:8-12,26-30).
 * x [M,K] with rows ldx floats apart, W [N,K] (torch.nn.Linear layout), y / dy [M,N] contiguous.
 * Backward: dW [N,K] = dy^T x, db [N] = column sums of dy (NULL: skipped), dx [M,K] = dy W (NULL:
 * skipped).  K % 4 == 0, N % 4 == 0.
 */
int rnnt_engine_linear_fwd(const float *x, int64_t ldx, const float *W, const float *bias, int M, int K,
                           int N, float *y, void *stream);
int rnnt_engine_linear_bwd_workspace_bytes(int M, int K, int N, size_t *out);
int rnnt_engine_linear_bwd(const float *x, int64_t ldx, const float *W, const float *dy, int M, int K,
                           int N, float *dx, float *dW, float *db, void *workspace, size_t ws_bytes,
                           void *stream);

/*
 * The same Linear layer (reference rnnt/joint.py:8-12,26-30: audio_ln / text_ln) on the f16x2 matrix pipes
 * (RNNT_DTYPE_F32_F16X2's arithmetic: three fp16 MFMA products of power-of-two-scaled, 2-way split operands, fp32
 * accumulation — the fp32 class of error): y = x W^T + b through the joint forward's pipeline as a plain GEMM, dx through
 * the same kernel on W^T, dW / db through the joint's dW kernel with dy and x as its two operands.  Operand scales are
 * found on the device every call.  Needs K % 128 == 0 and N % 128 == 0; x [M,K] rows ldx floats apart; W [N,K], dy [M,N],
 * y [M,N], dx [M,K] contiguous; bias / dx / db may be NULL.  `backward` selects the workspace of _bwd (W^T, operand planes,
 * split-K slabs) or of _fwd (the W pack).  Same ownership / stream / error rules as every other entry point.
 */
int rnnt_engine_linear_x2_workspace_bytes(int M, int K, int N, int backward, size_t *out);
int rnnt_engine_linear_x2_fwd(const float *x, int64_t ldx, const float *W, const float *bias, int M, int K,
                              int N, float *y, void *workspace, size_t ws_bytes, void *stream);
int rnnt_engine_linear_x2_bwd(const float *x, int64_t ldx, const float *W, const float *dy, int M, int K,
                              int N, float *dx, float *dW, float *db, void *workspace, size_t ws_bytes,
                              void *stream);

/*
 * The AudioEncoder's inference forward (reference rnnt/jasper.py:90-183, rnnt/causalconv.py:9-40; eval mode, fp32): mel
 * features to encoder output for a whole batch of utterances (rnnt_engine_encoder_fwd = AudioEncoder.forward) or for one
 * streaming push (rnnt_engine_encoder_stream_push = AudioEncoder.streaming_forward).  The module is handed over as a flat
 * list of layers in execution order, each  causal conv -> [norm] -> [+ residual branch] -> [exact GELU]:
 *     prologue (PLAIN);  per JasperBlock: its residual 1x1 (RESIDUAL: conv + norm of the block's input, kept aside), then
 *     its sub-blocks (FIRST .. PLAIN .. LAST; a block of one sub-block is FIRST | LAST; LAST adds the residual branch before
 *     its GELU);  epilogue (PLAIN);  the output 1x1 (FINAL: conv + bias only).
 * `cin` of a layer is `cout` of the layer before it (a RESIDUAL layer and the FIRST layer behind it read the same input; a
 * block's LAST `cout` is its RESIDUAL `cout`); layers inside a block have stride 1.
 *   weight [cout][cin][taps] (torch Conv1d), bias [cout]; gamma / beta [cout] or NULL (1 / 0); mean / var [cout]: the
 *   running statistics of RNNT_ENC_NORM_BATCH.  RNNT_ENC_NORM_INSTANCE takes mean and biased variance per (batch entry,
 *   channel) over the output frames of THIS call (so a streamed instance-norm encoder depends on the chunking, as the
 *   reference's does).
 * A conv of `taps` taps, stride s, dilation d reads X~ = state followed by the input frames; output frame t is
 * bias + sum_j sum_ci W[co][ci][j] X~[ci][t*s + j*d]; frames out = (len(X~) - d*(taps-1) - 1) / s + 1; the next state is X~
 * from frame out*s on.  A whole utterance starts from (taps-1)*d - s + 1 zero frames of state.
 *
 * rnnt_engine_encoder_pack writes the weights once as [tap][cout][cin rounded up to 4] per layer (only `weight` and the
 * dimensions are read); the other calls read `packed` and never `weight`.  Repack after the weights change.
 * x: N x cin x L fp32 with strides x_strides (floats; batch, channel, frame).  out: [N][L_out][cout of the last layer]
 * contiguous (time-major; L_out by the frame arithmetic above, layer after layer).  The last layer of the list stores there
 * whatever its role — a list need not end in FINAL; its norm, residual and GELU are what its role says.
 * Streaming: state_in / state_out are HOST arrays of n_layers device pointers, state_in_lens / state_out_lens HOST arrays
 * of n_layers frame counts (entries of RESIDUAL / FINAL layers are ignored); state i is (N, cin, len) contiguous fp32;
 * state_out_lens must be what the push leaves (checked), a state is never updated in place, a length of 0 needs no pointer.
 * regime: RNNT_ENC_REGIME_AUTO picks per layer the weight-streaming kernel (N * frames out <= 64 and N * len(X~) <= 224)
 * or the MFMA GEMM; RNNT_ENC_REGIME_MANY_ROWS forces the GEMM.  rnnt_engine_encoder_workspace_bytes: state_lens NULL = whole
 * utterance.  Results are bitwise reproducible.  RNNT_ERR_INVALID_ARG: null pointers, taps / stride / dilation < 1, an empty or
 * inconsistent layer list, too few frames for one output frame, a RNNT_ENC_NORM_INSTANCE layer with a single output frame
 * (no variance; the size query rnnt_engine_encoder_workspace_bytes refuses it as well); everything is checked before anything
 * is enqueued.
 */
#define RNNT_ENC_MAX_LAYERS 64
#define RNNT_ENC_NORM_NONE 0
#define RNNT_ENC_NORM_BATCH 1
#define RNNT_ENC_NORM_INSTANCE 2
#define RNNT_ENC_ROLE_PLAIN 0
#define RNNT_ENC_ROLE_FIRST 1
#define RNNT_ENC_ROLE_LAST 2
#define RNNT_ENC_ROLE_RESIDUAL 4
#define RNNT_ENC_ROLE_FINAL 8
#define RNNT_ENC_REGIME_AUTO 0
#define RNNT_ENC_REGIME_MANY_ROWS 1
typedef struct rnnt_encoder_layer {
    int cin, cout, taps, stride, dilation;
    int norm;  /* RNNT_ENC_NORM_* */
    int role;  /* RNNT_ENC_ROLE_* */
    float eps;
    const void *weight, *bias, *gamma, *beta, *mean, *var;
} rnnt_encoder_layer;
int rnnt_engine_encoder_packed_bytes(const rnnt_encoder_layer *layers, int n_layers, size_t *out);
int rnnt_engine_encoder_pack(const rnnt_encoder_layer *layers, int n_layers, void *packed, size_t packed_bytes, void *stream);
int rnnt_engine_encoder_workspace_bytes(const rnnt_encoder_layer *layers, int n_layers, int N, int L, int regime,
                                        const int32_t *state_lens, size_t *out);
int rnnt_engine_encoder_fwd(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                            const int64_t x_strides[3], int N, int L, int regime, float *out, void *workspace, size_t ws_bytes,
                            void *stream);
int rnnt_engine_encoder_stream_push(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                                    const int64_t x_strides[3], int N, int L, void *const *state_in, const int32_t *state_in_lens,
                                    void *const *state_out, const int32_t *state_out_lens, int regime, float *out, void *workspace,
                                    size_t ws_bytes, void *stream);

/*
 * The AudioEncoder's TRAINING forward and backward: whole utterances, fp32, exact fp32 products, the same flat
 * layer list.  Per layer, with X~ = lead[i] zero frames followed by the layer's input:
 *     y = conv(X~) + bias;  h = norm(y);  z = h (+ the residual branch on a LAST layer);  a = GELU(z) (RESIDUAL and FINAL
 *     layers: a = z);  o = a * keep / (1 - p) where keep[i] is given, else o = a.
 * RNNT_ENC_NORM_BATCH normalises with the running statistics (a frozen batch norm: gamma and beta get gradients, mean / var are
 * constants); batch statistics are not supported.  The backward follows from that definition; instance norm with the biased
 * variance: g = dz gamma, dy = rstd (g - mean_t g - xhat mean_t(g xhat)).  The gradient of x is not computed.
 *   lead  HOST array of n_layers frame counts: the zero frames in front of each conv's input,
 *         (taps-1)*dilation - stride + 1 - look-ahead; 0 <= lead[i] <= (taps-1)*dilation - stride + 1 is checked; entries of
 *         RESIDUAL / FINAL layers are ignored; NULL = no look-ahead anywhere.  Frames out = (lead + frames in -
 *         dilation*(taps-1) - 1) / stride + 1.  A block's LAST layer must leave as many frames as its RESIDUAL layer (the
 *         residual branch is added frame by frame): look-ahead inside a block is RNNT_ERR_INVALID_ARG.
 *   keep  HOST array of n_layers device pointers or NULL; keep[i] NULL: layer i drops nothing; else one byte per output value,
 *         [N][frames out][cout] contiguous, non-zero = kept.  A mask on a RESIDUAL / FINAL layer is refused.
 *   p     HOST array of n_layers drop probabilities in [0, 1) (read where keep[i] is given) or NULL = all 0.
 *   packed  rnnt_engine_encoder_train_pack: the forward's tables of rnnt_engine_encoder_pack for every layer, then per layer the
 *         dX conv's table [tap reversed][cin][cout rounded up to 4].  Repack after the weights change.
 *   saved   caller-owned, 16-byte aligned, rnnt_engine_encoder_train_saved_bytes; written by _train_fwd, read by _train_bwd.  Per
 *         layer, in list order, each piece rounded up to 256 bytes, rows of ld = cout rounded up to 4 floats:
 *           o    [N][frames out][ld]  the layer's output, the next layer's input    every layer but RESIDUAL ones and the list's last
 *           z    [N][frames out][ld]  the value in front of the GELU                every layer but RESIDUAL / FINAL ones
 *           xhat [N][frames out][ld]  the normalised conv output (y - mean) rstd    layers with a norm
 *           rstd [N][cout]                                                          RNNT_ENC_NORM_INSTANCE layers
 *         x, keep, p, lead and the layer list must be the forward's when _train_bwd runs.
 *   dout    [N][L_out][cout of the last layer] contiguous: the gradient of `out`.
 *   grads   HOST array of n_layers rnnt_encoder_grads; a NULL member is not computed; weight [cout][cin][taps], the others
 *         [cout].  They are written, not accumulated into.  gamma / beta of a layer without a norm are refused.
 * The workspace (rnnt_engine_encoder_train_workspace_bytes: the larger of both calls') carries nothing from _train_fwd to
 * _train_bwd.  `regime` picks the forward's conv kernel as above; the backward always runs the MFMA kernels.
 * Limits beside the inference entries': a layer behind the list's first (first two, where the list opens with a block) has
 * stride 1 (RNNT_ERR_UNSUPPORTED: dX exists for stride 1 only); N * frames in of every such layer <= 65535 * 32.
 * Launches per layer: forward 2 (conv, k_enc_norm<true>); backward 4 (k_enc_bwd_norm, k_enc_dw, k_enc_bwd_sum, the dX conv), 3
 * where the layer reads the list's input.  No atomics; every sum has a fixed order: results are bitwise reproducible.
 * Everything is checked before anything is enqueued.
 */
typedef struct rnnt_encoder_grads {
    void *weight, *bias, *gamma, *beta;
} rnnt_encoder_grads;
int rnnt_engine_encoder_train_packed_bytes(const rnnt_encoder_layer *layers, int n_layers, size_t *out);
int rnnt_engine_encoder_train_pack(const rnnt_encoder_layer *layers, int n_layers, void *packed, size_t packed_bytes, void *stream);
int rnnt_engine_encoder_train_saved_bytes(const rnnt_encoder_layer *layers, int n_layers, int N, int L, const int32_t *lead,
                                          size_t *out);
int rnnt_engine_encoder_train_workspace_bytes(const rnnt_encoder_layer *layers, int n_layers, int N, int L, int regime,
                                              const int32_t *lead, size_t *out);
int rnnt_engine_encoder_train_fwd(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                                  const int64_t x_strides[3], int N, int L, const int32_t *lead, const void *const *keep,
                                  const float *p, int regime, float *out, void *saved, size_t saved_bytes, void *workspace,
                                  size_t ws_bytes, void *stream);
int rnnt_engine_encoder_train_bwd(const rnnt_encoder_layer *layers, int n_layers, const void *packed, const float *x,
                                  const int64_t x_strides[3], int N, int L, const int32_t *lead, const void *const *keep,
                                  const float *p, const float *dout, const void *saved, size_t saved_bytes,
                                  const rnnt_encoder_grads *grads, void *workspace, size_t ws_bytes, void *stream);

/*
 * The audio featurizer (reference rnnt/featurizer.py): samples to the features the encoder reads.  Frame f,
 * bin k (n_fft / 2 + 1 bins) of utterance n:
 *     p = | sum_j w[j] x[f * hop_length + j] exp(-2 pi i j k / n_fft) |^2        (torch.stft, onesided, not normalized)
 *     with n_filters > 0:  p[m] = sum_k p[k] fbank[k][m]                         (fbank: n_freq x n_filters fp32, row-major)
 *     v = log(p + 1e-6)                                  RNNT_FEAT_LOG_PLAIN
 *         p > 0.01 ? log p : 50 p + log(0.01) - 0.5      RNNT_FEAT_LOG_PIECEWISE
 *         log((p + 1e-6) gain)                           RNNT_FEAT_LOG_GAIN
 *     out[n * s0 + k * s1 + f * s2] = (v - mean[k]) * invstd[k]                  (mean, invstd: F floats on the device,
 *                                                                                 F = n_filters, or the bins without one)
 * The window (win_length fp32 values on the device) is centred in n_fft with zeros, as torch.stft does.  center = 1 reflects
 * n_fft / 2 samples at both ends.  Frames per utterance of `len` samples, host arithmetic: (len - n_fft) / hop + 1 (0 below
 * n_fft), or (len + 2 (n_fft / 2) - n_fft) / hop + 1 with center (integer divisions: len / hop + 1 for an even n_fft).
 *
 * rnnt_engine_featurizer_pack writes the windowed DFT basis once (rnnt_engine_featurizer_basis_bytes; 16-byte aligned); the
 * other calls read it.  rnnt_engine_featurizer_fwd: N waveforms of T samples, wave_stride samples apart, fp32
 * (RNNT_FEAT_PCM_F32) or int16 scaled by 1 / 32768 (RNNT_FEAT_PCM_S16); `lens`: HOST array of N sample counts (0 .. T), or
 * NULL = all T.  `out` holds L frames per utterance through out_strides (floats; batch entry, bin, frame): L is at least the
 * longest utterance's frame count (checked), frames from an utterance's own count up to L are stored as zeros.  workspace:
 * rnnt_engine_featurizer_workspace_bytes(desc, N, L) — 0 without a filterbank, NULL is then fine.
 * rnnt_engine_featurizer_stream_push: one push of N streams; X~ = state_in (N x state_in_len fp32, contiguous) followed by
 * the chunk (N x T).  L must be the frames X~ completes and state_out_len what it leaves, len(X~) - L * hop_length (both
 * checked; HOST ints); state_out (N x state_out_len fp32) is X~ from sample L * hop_length on and is never state_in.  A push
 * that completes no frame is valid (L = 0, out may be NULL).  T = 0 is valid.  center = 1 is refused.
 * Every (bin, frame) is summed in one fixed order: results are bitwise reproducible and a streamed utterance equals the whole
 * one bit for bit.  No atomics, no host synchronisation.  RNNT_ERR_INVALID_ARG: null pointers, hop_length < 1,
 * win_length > n_fft, odd n_fft - win_length, a reflect pad not shorter than the utterance, a wrong L or state length;
 * RNNT_ERR_UNSUPPORTED: 31 hop_length + n_fft samples beyond the kernel's 64 KB stage, a stream with hop_length > n_fft
 * (samples between frames would be skipped, not carried).  Everything is checked before
 * anything is enqueued.
 */
#define RNNT_FEAT_LOG_PLAIN 0
#define RNNT_FEAT_LOG_PIECEWISE 1
#define RNNT_FEAT_LOG_GAIN 2
#define RNNT_FEAT_PCM_F32 0
#define RNNT_FEAT_PCM_S16 1
typedef struct rnnt_featurizer_desc {
    int n_fft, win_length, hop_length;
    int center;   /* 0 or 1 */
    int log_kind; /* RNNT_FEAT_LOG_* */
    float gain;   /* RNNT_FEAT_LOG_GAIN */
    int n_filters; /* 0: no filterbank */
} rnnt_featurizer_desc;
int rnnt_engine_featurizer_basis_bytes(const rnnt_featurizer_desc *desc, size_t *out);
int rnnt_engine_featurizer_pack(const rnnt_featurizer_desc *desc, const float *window, void *basis, size_t basis_bytes, void *stream);
int rnnt_engine_featurizer_workspace_bytes(const rnnt_featurizer_desc *desc, int N, int L, size_t *out);
int rnnt_engine_featurizer_fwd(const rnnt_featurizer_desc *desc, const void *basis, const void *fbank, const void *wave,
                               int64_t wave_stride, int N, int T, const int32_t *lens, int pcm, const float *mean,
                               const float *invstd, float *out, const int64_t out_strides[3], int L, void *workspace,
                               size_t ws_bytes, void *stream);
int rnnt_engine_featurizer_stream_push(const rnnt_featurizer_desc *desc, const void *basis, const void *fbank,
                                       const float *state_in, int state_in_len, const void *chunk, int64_t chunk_stride, int N, int T,
                                       int pcm, const float *mean, const float *invstd, float *out, const int64_t out_strides[3],
                                       int L, float *state_out, int state_out_len, void *workspace, size_t ws_bytes, void *stream);

/*
 * Multi-GPU step of the path (the suggested export of 8b): ONE sum all-reduce, in
 * place, of `count` fp32 values — the flat [dW (V*H) | db (V) | loss] buffer of a batch-sharded
 * step — on the caller's RCCL communicator (`comm` is an ncclComm_t) and stream.  Stands where the
 * reference relies on DDP's gradient all-reduce (rnnt/train.py:28,68: backend "nccl" = RCCL on
 * ROCm).  The engine does not link RCCL: ncclAllReduce is resolved at call time from the RCCL the
 * process already has loaded (PyTorch's), else from librccl.so.1 on the loader path; it creates no
 * communicator and keeps none.  Returns RNNT_ERR_UNSUPPORTED when no RCCL can be found,
 * RNNT_ERR_LAUNCH with RCCL's message when the collective fails.
 */
int rnnt_engine_allreduce(void *buf, size_t count, void *comm, void *stream);

/*
 * Diagnostic view of the last fused call's intermediate buffers inside `workspace`
 * (offsets in bytes; valid for the dims given).  Used by tests and bench.py to time or
 * inspect single stages; not needed by training code.
 */
typedef struct rnnt_engine_ws_layout {
    size_t logits, hidden, denom_s, lpb_s, lpe_s, alpha_s, beta_s, coef, wpack, enc_copy;
    size_t slab_enc, slab_pred, slab_w, slab_b, counters, total, rows_pad;
    int n_ublk, n_ttile, n_split, D;
    size_t g_lo;          /* RNNT_DTYPE_F32_BF16X3: lo plane of G */
    size_t aux, aux_bytes; /* RNNT_DTYPE_F32_BF16X3: fp32 hidden + W pack of the RNNT_VARIANT_X3_FP32_* stages, placed BEHIND
                            * `total` (aux == total): only a call with such a variant needs total + aux_bytes */
    size_t ep;            /* RNNT_DTYPE_F32_F16X2: exp(2 enc) [B][H/16][T][16] then exp(2 pred) [B][H/16][U1][16], fp32 (0: none) */
    size_t x2_live;       /* RNNT_DTYPE_F32_F16X2 (0: none): the live structures of the last call's backward.  At +0 six int32 counts:
                           * live 16-cell dW k-steps, k-steps that hold a cell, live dHidden tiles (8 t x 16 u), dHidden tiles, live 4-cell
                           * dW groups, groups that hold a cell; at +256 one byte per dHidden tile [B][ceil(T/8)][ceil(U1/16)], 1 = live (the
                           * k-step bitmap and list, the tile list, the group bitmap and list follow) */
} rnnt_engine_ws_layout;

int rnnt_engine_workspace_layout(int B, int T, int U1, int H, int V, int dtype,
                                 rnnt_engine_ws_layout *out);

/*
 * Run ONE stage of the fused pipeline on an already laid-out workspace (bench/profiling
 * aid: lets bench.py time the dominant kernels with HIP events on the launch stream).
 * stage: 0 operand producers (hidden = tanh(enc+pred), W repack), 1 joint-forward GEMM kernel,
 * 2 lattice sweep (alpha & beta), 3 gradient coefficients + G in place of logits, 4 dHidden GEMM
 * kernel, 5 dEnc/dPred slab reduction, 6 dW GEMM kernel, 7 dW/db slab reduction.
 * Arguments as for rnnt_engine_joint_loss_fwd_bwd.
 */
int rnnt_engine_run_stage(int stage, const void *enc, const int64_t enc_strides[3],
                          const void *pred, const void *W, const void *bias,
                          const int32_t *targets, const int32_t *logit_lens,
                          const int32_t *target_lens, int B, int T, int U1, int H, int V,
                          int blank, float clamp, float grad_scale, int dtype, float *costs,
                          void *grad_enc, void *grad_pred, void *grad_W, void *grad_bias,
                          void *workspace, size_t ws_bytes, void *stream);

/*
 * Any subset of the stages (bit s of `stage_mask` = stage s above; 255 = the whole pipeline) with
 * the kernel variants of `variant` (RNNT_VARIANT_*), chosen for this call only.  Gradient
 * pointers may be NULL when no backward stage (4..7) is selected.  Test / bench aid.
 */
int rnnt_engine_run_stages(int stage_mask, int variant, const void *enc, const int64_t enc_strides[3],
                           const void *pred, const void *W, const void *bias, const int32_t *targets,
                           const int32_t *logit_lens, const int32_t *target_lens, int B, int T, int U1,
                           int H, int V, int blank, float clamp, float grad_scale, int dtype,
                           float *costs, void *grad_enc, void *grad_pred, void *grad_W,
                           void *grad_bias, void *workspace, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RNNT_ENGINE_H */
