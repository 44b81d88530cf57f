/* tethys_mi.h — C ABI of libtethys_mi.so: the MI355X (gfx950) kernels behind the
 * tethys-speech data-parallel training step.
 *
 * The reference (hyunnnchoi/tethys-speech) has NO plugin / FFI interface: its hot path is
 * stock TensorFlow ops called from speech_jobs/whisper_dist.py and
 * speech_jobs/wav2vec2_dist.py.  Each entry point below therefore cites the
 * TensorFlow call site(s) in those files whose device arithmetic it replaces
 * ("W:" = speech_jobs/whisper_dist.py, "V:" = speech_jobs/wav2vec2_dist.py).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless noted;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it;
 *   - no allocation, no synchronisation, no hidden state inside any call: the caller owns
 *     every buffer including workspaces (sizes documented per call);
 *   - return value: 0 = TMI_OK, negative = TMI_ERR_*; never throws, never exits;
 *   - dtype enum: TMI_F32 / TMI_BF16; every reduction accumulates in fp32.
 */
#ifndef TETHYS_MI_H
#define TETHYS_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMI_OK 0
#define TMI_ERR_INVALID (-1)   /* bad argument (shape, alignment, dtype combination) */
#define TMI_ERR_LAUNCH (-2)    /* hipLaunchKernel reported an error */
#define TMI_ERR_UNSUPPORTED (-3)
#define TMI_ERR_CALLBACK (-4)  /* tmi_plan_replay: a callback node returned non-zero; the nodes after it were not issued */

#define TMI_F32 0
#define TMI_BF16 1

/* ABI version, bumped on any signature change. */
int tmi_abi_version(void);
/* Last HIP error string seen by a launch in this thread (host pointer, static storage). */
const char* tmi_last_error(void);
/* Reproducible reductions, process-wide, read at launch time (returns the previous setting).  On: tmi_colsum runs one
 * workgroup per column group and every library-chosen split-K that has to fall back to fp32 atomics is capped at two
 * contributions per element (a + b = b + a; splits through workspace slabs are ordered anyway), so no result of those
 * kernels depends on arrival order; callers pair it with the workspace (fixed-order fold) form of tmi_layernorm_bwd.
 * Scope: the kernels of the WHISPER step - the Wav2Vec2 kernels that sum with atomics (GroupNorm parameter and codebook
 * gradients) are not covered.  With both, a Whisper step is bit-reproducible (the reference,
 * TensorFlow on GPU, is not run-to-run reproducible either: no file:line to cite - this is a property the parity tests
 * use, tests/test_whisper_step_gpu.py). */
int tmi_set_deterministic(int on);

/* ------------------------------------------------------------------------------------
 * Strided, batched GEMM with fused epilogue.  Replaces every tf.keras.layers.Dense call
 * (W:89-92 q/k/v/out_proj, W:194-197 fc1/fc2, W:545 lm_head) and, through overlapping-row
 * addressing of a channels-last padded buffer, tf.keras.layers.Conv1D (W:311-312) and the
 * backward matmuls tape.gradient (W:833) derives from them.
 *
 *   for b in [0,nbatch):  C_b[m,n] = epi( sum_{kb<kbatch} sum_{k<K} A(b,kb,m,k) * B(b,kb,k,n) )
 *   A(b,kb,m,k) = A[b*a_sb + kb*a_skb + m*a_sm + k*a_sk]      (element strides)
 *   B(b,kb,k,n) = B[b*b_sb + kb*b_skb + k*b_sk + n*b_sn]
 *   C_b[m,n]    = C[b*c_sb + m*ldc + n]
 * epi(v), applied in this order:
 *   v += bias[b*bias_sb + n]          (bias f32 or NULL; bias_sb = 0 shares one bias over the batch)
 *   if n < scale_cols: v *= scale     (W:141: q = (xWq+b) * head_dim^-0.5)
 *   v += C_old                        (if accumulate != 0)
 *   if aux_out: aux_out[..] = v       (pre-activation saved for backward; layout as C)
 *   if act == 1: v = gelu_erf(v)      (tf.keras.activations.gelu, W:195,333,336)
 *   if aux_in:  v *= gelu_erf'(aux_in[..])   (backward through GELU; layout as C)
 *   if resid:   v += resid[b*r_sb + m*r_ld + n]  (residual add W:228,234 / PE add W:339)
 * splitk > 1 partitions the (kb,k) range over extra workgroups and accumulates with
 * fp32 atomics into a PRE-ZEROED fp32 C (no epilogue terms allowed); splitk == 0 lets the
 * library choose (it only splits epilogue-free fp32-output GEMMs, i.e. weight gradients, and
 * then C must be pre-zeroed); splitk == 1 never splits.
 * workspace (optional scratch in device memory, contents irrelevant, owned by the call while it
 * runs on its stream; TMI_GEMM_WORKSPACE_MIN bytes always suffice): when given, a library-chosen
 * split (splitk == 0) of a long reduction is reduced WITHOUT atomics — every split runs the epilogue
 * into its own fp32 slab there and a streaming pass sums the slabs into C, so fp32 atomics (~0.5 TB/s on
 * MI355X) leave the path and that launch does not read C.  Which launches go through the slabs is the library's choice
 * (long reductions on the fast kernels; short ones, and every split of the generic kernel of csrc/gemm.hip - operands that
 * miss the fast kernels' alignment, TMI_GEMM_GENERIC=1 - still use atomics), so a caller of splitk == 0 without
 * `accumulate` pre-zeroes C whether it passes a workspace or not: the step does (tests/test_gemm_forced_gpu.py runs the
 * same launches on every kernel and found the generic kernel summing into whatever C held).
 * Operand padding: a k-strided operand (row stride >= round_up(cols, 8)) is read in whole 16-byte chunks, and the padding
 * columns cols .. round_up(cols, 8) - 1 may hold anything, NaN included - they only reach accumulator rows / columns that are
 * never stored (tests/test_gemm_forms_gpu.py poisons them).
 * in_dtype: type of A and B; out_dtype: type of C, aux_*, resid.  Valid pairs:
 * (F32,F32), (BF16,BF16), (BF16,F32).  fp32 inputs use the exact-fp32 MFMA
 * (v_mfma_f32_32x32x2_f32); bf16 inputs use v_mfma_f32_32x32x16_bf16.
 */
#define TMI_GEMM_WORKSPACE_MIN (96ll << 20)
typedef struct tmi_gemm_desc {
  const void* A; const void* B; void* C;
  int64_t M, N, K;
  int64_t a_sm, a_sk, b_sk, b_sn, ldc;
  int64_t nbatch, a_sb, b_sb, c_sb;
  int64_t kbatch, a_skb, b_skb;
  const float* bias; int64_t bias_sb;
  int64_t scale_cols; float scale;
  int32_t accumulate;
  int32_t act;
  void* aux_out; const void* aux_in;
  const void* resid; int64_t r_ld, r_sb;
  int32_t splitk;
  int32_t in_dtype, out_dtype;
  void* workspace; int64_t workspace_bytes;
  /* Dropout on the epilogue value, before the residual add (W:205: x + Dropout(fc2(..)); V:396, V:431):
   * C = resid + (keep ? v / (1 - p) : 0) with the generator of tmi_dropout over the [M, N] output (row m, column n; N <= 2^17).
   * dropout_p == 0 is off.  nbatch must be 1. */
  float dropout_p; uint64_t dropout_seed;
  /* A second, OUTER batch level (0 / 1 = none): problem z = b2 * nbatch + b1 reads A + b1*a_sb + b2*a_sb2 (likewise B, C).
   * For operands whose two batch indices are not one stride apart - per-(sample, head) products on [B, T, H*hd] tensors
   * (W:147-167 in the fp32 parity mode: one launch instead of one per sample).  Only with plain epilogues (scale /
   * accumulate), nbatch * nbatch2 <= 65535; never on the bf16 fast path. */
  int64_t nbatch2, a_sb2, b_sb2, c_sb2;
} tmi_gemm_desc;
int tmi_gemm(const tmi_gemm_desc* d, void* stream);
/* Diagnostic, host only: which kernel the last tmi_gemm launched from the calling thread ran on (0: none yet) - the
 * numbering of the TMI_GEMM_CFG switch (csrc/gemm_fast.hip: 4, 5, 6, 12, 13, 15, 16 the bf16 tiles, 10 / 14 the eight-phase
 * kernel with 256- / 192-row tiles), TMI_GEMM_KERNEL_F32 the fp32-operand kernel, TMI_GEMM_KERNEL_GENERIC the kernel of
 * csrc/gemm.hip.  *nsplit: the number of K ranges (1 = no split); *flags: TMI_GEMM_PATH_* bits.  Either may be NULL.
 * The record is written just before the launch; the tests assert it, so that a dispatch threshold that moves shows up as
 * a failed expectation instead of as lost coverage. */
#define TMI_GEMM_KERNEL_GENERIC 1
#define TMI_GEMM_KERNEL_F32 32
#define TMI_GEMM_PATH_PERSISTENT 1   /* eight-phase kernel, 256 workgroups walking the tile slots */
#define TMI_GEMM_PATH_ATOMIC 2       /* split-K summed with fp32 atomics into C */
#define TMI_GEMM_PATH_SLABS 4        /* split-K through workspace slabs and the reduce pass */
#define TMI_GEMM_PATH_XCD_GROUPS 8   /* the 2 / 4 / 8 K ranges dealt over groups of XCDs */
#define TMI_GEMM_PATH_XCD_DEAL 16    /* eight-phase kernel, 16 / 32 K ranges, two / four per XCD */
#define TMI_GEMM_PATH_WIDE 32        /* 16-byte epilogue accesses (clear: element by element) */
int tmi_gemm_last_path(int32_t* nsplit, int32_t* flags);

/* ------------------------------------------------------------------------------------
 * LayerNorm over the last axis of x[rows, C].  Replaces
 * tf.keras.layers.LayerNormalization(epsilon=1e-5) (W:214,216,245,249,253,322,392) and
 * its gradient.  mean/rstd are fp32 [rows], saved for backward.
 * Backward: dgamma[C] / dbeta[C] are ACCUMULATED into (the caller zeroes them); dx = (accumulate_dx ? dx : 0) + dLN/dx.
 * `workspace` (fp32, 16-byte aligned, >= tmi_layernorm_bwd_workspace_bytes(rows, C, emit) bytes, the caller's): every
 * workgroup stores its partial column sums there and a second launch on the same stream adds them in workgroup order -
 * no atomics, bit-reproducible, no slow-down beside other kernels.  workspace == NULL: one fp32 atomic per column per
 * workgroup (order-dependent last bits; serialises at the memory side under load).
 */
int tmi_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* y,
                      float* mean, float* rstd, int64_t rows, int64_t C, float eps,
                      int32_t dtype, void* stream);
/* Dropout(LayerNorm(x)) in one pass and its gradient (V:296, V:560, V:779: `layer_norm` then `dropout`): the forward applies
 * the flat dropout generator (tmi_dropout: stream 0, row, column of the [rows, C] output) to y on store; the backward
 * applies the same mask to dy on load (the same seed), then runs tmi_layernorm_bwd.  dropout_p = 0: the plain entries. */
int tmi_layernorm_dropout_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                              int64_t rows, int64_t C, float eps, float dropout_p, uint64_t dropout_seed, int32_t dtype,
                              void* stream);
int tmi_layernorm_dropout_bwd(const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                              void* dx, float* dgamma, float* dbeta, int64_t rows, int64_t C, int32_t accumulate_dx,
                              float dropout_p, uint64_t dropout_seed, float* workspace, int64_t workspace_bytes,
                              int32_t dtype, void* stream);
int64_t tmi_layernorm_bwd_workspace_bytes(int64_t rows, int64_t C, int32_t emit);
int tmi_layernorm_bwd(const void* dy, const void* x, const float* gamma, const float* mean,
                      const float* rstd, void* dx, float* dgamma, float* dbeta, int64_t rows,
                      int64_t C, int32_t accumulate_dx, float* workspace, int64_t workspace_bytes,
                      int32_t dtype, void* stream);

/* tmi_layernorm_bwd that also emits what the Dense layer BELOW this LayerNorm's residual stream needs from dx (the
 * gradient this kernel writes is that layer's dy): colsum[c] += sum over rows of dy' (its bias gradient), where
 * dy' = dx, or - when that layer's output went through Dropout (W:205, V:396, V:431) - dy' = mask * dx / (1 - p), which is
 * also written to `masked` [rows][C] (the generator of tmi_dropout over [rows, C] with `dropout_seed`).  masked == NULL:
 * no copy, column sums of dx; masked != NULL with dropout_p == 0: column sums of dx and a plain second copy of dx in
 * `masked` (a snapshot for a weight gradient launched after dx has been overwritten).  Replaces a tmi_dropout and a
 * tmi_colsum pass over dx. */
int tmi_layernorm_bwd_emit(const void* dy, const void* x, const float* gamma, const float* mean,
                           const float* rstd, void* dx, float* dgamma, float* dbeta, int64_t rows,
                           int64_t C, int32_t accumulate_dx, float* colsum, void* masked,
                           float dropout_p, uint64_t dropout_seed, float* workspace,
                           int64_t workspace_bytes, int32_t dtype, void* stream);

/* out[n] += sum over rows of dY[rows, N] (row stride ld): the bias gradient of a Dense /
 * Conv1D layer.  Accumulates with fp32 atomics (one per column per workgroup); the caller
 * zeroes `out`. */
int tmi_colsum(const void* dy, int64_t ld, float* out, int64_t rows, int64_t N,
               int32_t dtype, void* stream);
/* nbatch matrices dy + b * dy_sb (elements) into nbatch vectors out + b * out_sb in one launch: the bias gradients of the
 * same Dense layer in every transformer layer (deferred, batched weight gradients). */
int tmi_colsum_batched(const void* dy, int64_t ld, int64_t dy_sb, float* out, int64_t out_sb,
                       int64_t rows, int64_t N, int64_t nbatch, int32_t dtype, void* stream);

/* dx = dy * gelu_erf'(u), elementwise over n elements (backward of W:336 where the GELU
 * output feeds the positional add rather than a GEMM). */
int tmi_gelu_bwd(const void* dy, const void* u, void* dx, int64_t n, int32_t dtype, void* stream);
/* The same over nbatch spans of n elements whose starts are dy_sb / u_sb / dx_sb elements apart (one
 * launch for the per-sample spans of a padded buffer). */
/* Dropout (tf.keras.layers.Dropout in training, W:205 / W:342 / W:411) over a [rows, cols] tensor, cols even and
 * <= 2^17:
 *   out[r,c] = (resid ? resid[r,c] : 0) + (keep(seed, r, c) ? in[r,c] * 65536/(65536-thr) : 0),
 * thr = round(p * 65536): element (r, c) is dropped when its 16-bit draw (low / high half, for even / odd c, of one
 * 32-bit hash of (row key of (seed, r), c>>1)) is below thr.  Nothing is stored: the backward applies the same call (same seed) to the
 * incoming gradient.  TF's RNG stream cannot be reproduced, so the mask differs from the reference's; the oracle
 * restates this generator (oracle/dropout.py).  out may alias in. */
int tmi_dropout(const void* in, int64_t ld_in, const void* resid, int64_t ld_res, void* out, int64_t ld_out,
                int64_t rows, int64_t cols, float p, uint64_t seed, int32_t dtype, void* stream);
int tmi_gelu_bwd_batched(const void* dy, const void* u, void* dx, int64_t n, int64_t nbatch, int64_t dy_sb,
                         int64_t u_sb, int64_t dx_sb, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Launch plans: record the launches of one training step once, replay them from ONE call.
 * Replaces what `@tf.function` gives the reference's step (W:818-819: the first call traces the step, every later call
 * replays the traced graph with no Python between its ops).  While a plan records (tmi_plan_begin .. tmi_plan_end, on the
 * calling thread) every launching entry point of this header appends itself, with its arguments copied by value, to the
 * plan and then runs as usual: the recorded step is a real step.  tmi_plan_replay issues the recorded calls in order -
 * the same entry points, argument checks and dispatch rules, no host code in between - adding `seed_delta` to every
 * recorded dropout seed (site seeds are base + step * K + site * K': pass (step_now - step_recorded) * K mod 2^64) and
 * `step_delta` to the `step` argument of tmi_adam_step / _rows / _segments.
 * Ordering between streams is part of the plan: the host reports each event record / stream wait it makes while recording
 * (tmi_plan_note_event_record / tmi_plan_note_stream_wait, raw hipEvent_t / hipStream_t handles that must outlive the
 * plan) and the replay repeats them with hipEventRecord / hipStreamWaitEvent.  tmi_plan_note_callback records a host
 * function called in sequence (what a step does between launches that is not this library's: an RCCL collective);
 * it returns 0 to go on, and anything else ends the replay at once: no later node is issued and tmi_plan_replay
 * returns TMI_ERR_CALLBACK (a failed exchange must not be followed by the Adam updates on unreduced gradients).
 * Memory operations of a step go through tmi_memset_async / tmi_memset2d_async / tmi_memcpy_async (device to device)
 * so that they are recorded too.  tmi_plan_size: what = 0 nodes, 1 launches, 2 event-record nodes, 3 stream-wait
 * nodes, 4 callback nodes (-1 for anything else).  One recorder per thread; a plan is replayed by one thread at a time.
 */
typedef struct tmi_plan tmi_plan;
int tmi_plan_create(tmi_plan** out);
int tmi_plan_destroy(tmi_plan* plan);
int tmi_plan_begin(tmi_plan* plan);
int tmi_plan_end(tmi_plan* plan);
int tmi_plan_replay(tmi_plan* plan, uint64_t seed_delta, int64_t step_delta);
int64_t tmi_plan_size(const tmi_plan* plan, int32_t what);
int tmi_plan_note_event_record(void* event, void* stream);
int tmi_plan_note_stream_wait(void* stream, void* event);
int tmi_plan_note_callback(int (*fn)(void));
int tmi_memset_async(void* dst, int32_t value, int64_t bytes, void* stream);
int tmi_memset2d_async(void* dst, int64_t pitch_bytes, int32_t value, int64_t width_bytes, int64_t rows, void* stream);
int tmi_memcpy_async(void* dst, const void* src, int64_t bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Materialised-score softmax (fp32 "parity mode" attention, the reference's own graph
 * shape: W:147-167).  s[rows, Tk] in place; row r belongs to query i = r % Tq.
 * mask_mode 0: none.  mask_mode 1: the reference decoder's additive mask
 * (1 - (1 - band_part(ones,-1,0))) * -1e9 (W:416-418, W:152-153): key j <= i gets -1e9
 * added in fp32, keys j > i are left alone.
 * Backward: ds = p * (dp - sum_j p*dp), dp in place.
 */
int tmi_softmax_fwd(float* s, int64_t rows, int64_t Tq, int64_t Tk, int32_t mask_mode, void* stream);
int tmi_softmax_bwd(const float* p, float* dp, int64_t rows, int64_t Tk, void* stream);
/* The same materialised softmax with the additive key term of tmi_attn_desc.mask_mode 2 (V:352-355): s[rows, Tk] in place,
 * rows = B * H * Tq, row r belongs to batch r / (H * Tq); key j of batch b gets key_bias[b * kb_sb + j] (fp32, natural-log
 * units) added in fp32 before the row maximum is taken.  Forward only (inference). */
int tmi_softmax_bias_fwd(float* s, int64_t rows, int64_t Tq, int64_t Tk, int64_t H, const float* key_bias, int64_t kb_sb,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * Fused (flash-style) multi-head attention, bf16 in / fp32 accumulate, head_dim 64.
 * Replaces W:147-171 (scores, mask, softmax, probs @ v, head merge) without ever
 * materialising [B,H,Tq,Tk].  q/k/v/o are addressed as  ptr[b*sb + t*st + h*64 + d]
 * (element strides), so q, k, v may be column slices of one fused QKV buffer.
 * The query is expected pre-scaled (tmi_gemm scale_cols), as in W:141.
 * stats: fp32 [B,H,Tq,2] = (row max m, 1/row sum) — kept separately because with the
 * reference's -1e9 mask a fully masked row has m = -1e9, where m + log(l) is not
 * representable in fp32.
 * Backward is two kernels (no atomics, deterministic): dq pass owns query rows, dkv pass
 * owns key rows; both recompute p from q, k and stats.  delta[B,H,Tq] = rowsum(do * o) is
 * produced by tmi_attn_bwd itself into `delta` (fp32 workspace).
 */
typedef struct tmi_attn_desc {
  const void* q; const void* k; const void* v; void* o;
  int64_t q_sb, q_st, k_sb, k_st, v_sb, v_st, o_sb, o_st;
  float* stats;
  int64_t B, H, Tq, Tk;
  int32_t mask_mode;           /* 0, 1: as tmi_softmax_fwd; 2: additive key_bias (below), forward only */
  /* backward only */
  const void* d_o; void* dq; void* dk; void* dv;
  int64_t do_sb, do_st, dq_sb, dq_st, dk_sb, dk_st, dv_sb, dv_st;
  float* delta;
  float dq_scale;              /* dq is multiplied by this on store (chain rule of W:141) */
  float score_scale;           /* scores = (q . k) * score_scale (V:349 divides AFTER q.k^T); 0 means 1 */
  /* Dropout on the attention probabilities (W:160), training mode: 0 <= dropout_p < 1, 0 = off.  The keep
   * mask is a function of (dropout_seed, b, head, q, k) (tmi_common.h: tmi_keep_attn; oracle/dropout.py keep_attention);
   * the row sums that normalise the probabilities are taken before dropping, as tf.nn.softmax -> Dropout does.
   * TensorFlow draws the mask once and keeps it for the gradient (W:160): so does this pair of entry points -
   * tmi_attn_fwd evaluates the generator and stores 1 keep bit per score into `drop_mask`, tmi_attn_bwd reads the
   * bits and never hashes.  drop_mask: 16-byte aligned device buffer of tmi_attn_dropmask_bytes(B, H, Tq, Tk) bytes
   * owned by the caller from the forward call to the backward call of the same descriptor; required when
   * dropout_p > 0 (TMI_ERR_INVALID otherwise), ignored when dropout_p == 0.  Layout (private to the two entry
   * points): u32 words [B*H][ceil(Tk/64)][2][ceil(Tq/128)*128], one word = the 32 keys a forward lane holds of one
   * 64-key tile. */
  float dropout_p;
  uint64_t dropout_seed;
  void* drop_mask;
  int64_t drop_mask_bytes;
  /* Optional fp32 scratch (16-byte aligned, tmi_attn_workspace_bytes(B, H, Tq) bytes; NULL = none).  With it, the forward
   * and dQ passes of a short query side against a long key side (one query tile, >= 8 key tiles of 64, mask_mode 0: the
   * cross-attention of W:255-301) split the keys over 2-4 workgroups per (batch, head) and fold the partials in a second
   * launch: the lone 100-row query tile is otherwise one latency chain of 24 key tiles on 96 of 256 CUs. */
  void* workspace;
  int64_t workspace_bytes;
  /* tmi_attn_bwd only.  0 or 3: both passes (ONE launch when Tq <= 256 and Tk <= 256 - the dK/dV workgroups then compute the
   * row sums themselves, in the dQ pass's order: the outputs and `delta` are bit for bit those of the two launches); 1: the dQ
   * pass alone (it also fills `delta`); 2: the dK/dV pass alone, after a dQ pass of the same descriptor has filled `delta`.  Lets a caller put the dK/dV pass of a cross-attention - whose results
   * nothing on the decoder's backward chain waits for (W:255-301: dK, dV feed the shared k/v projections) - on another stream. */
  int32_t bwd_passes;
  /* mask_mode 2, tmi_attn_fwd only (the padding mask of a batch of clips of different lengths, V:352-355): the score of
   * (b, head, q, key) is q.k * score_scale + key_bias[b * kb_sb + key].  fp32, natural-log units, the same for every head
   * and query; the caller passes the reference's (1 - attention_mask) * -10000.  The term is finite, so a row whose keys
   * all carry it is an ordinary softmax of shifted scores, as in the reference.  Required (non-NULL, kb_sb >= 0) with
   * mask_mode 2 and ignored otherwise; mask_mode 2 with dropout_p > 0, and tmi_attn_bwd with mask_mode 2, return
   * TMI_ERR_INVALID.  The key-split path (`workspace`) is never taken.  Callers of mask_mode 0 / 1 leave both fields zero. */
  const float* key_bias;
  int64_t kb_sb;
} tmi_attn_desc;
int64_t tmi_attn_workspace_bytes(int64_t B, int64_t H, int64_t Tq);
int64_t tmi_attn_dropmask_bytes(int64_t B, int64_t H, int64_t Tq, int64_t Tk);
int tmi_attn_fwd(const tmi_attn_desc* d, void* stream);
int tmi_attn_bwd(const tmi_attn_desc* d, void* stream);
/* The attention weights of a call tmi_attn_fwd has made (the reference's `attention_probs`, W:176 / V:376; inference:
 * output_attentions): probs[(b*H + h)*p_sbh + q*p_sq + key] = softmax(scores)[b, h, q, key] for q < Tq, key < Tk, and
 * nothing else is written.  One launch recomputes the scores from q and k exactly as the backward passes do and
 * normalises them with `stats` as tmi_attn_fwd left them for the same descriptor (key-split or not), so the result is
 * the forward's own normalisation: x = q.k * score_scale * log2(e) (+ the fp32 -1e9 * log2(e) for keys j <= i in
 * mask_mode 1, + key_bias * log2(e) in mask_mode 2), p = exp2(x - m) * (1/l).  It is the probability BEFORE dropout.
 * Reads q, k with their strides, stats, B, H, Tq, Tk, mask_mode (0, 1, 2), score_scale, key_bias / kb_sb; v, o, the
 * backward fields and the workspace are ignored.  probs_dtype: TMI_F32 or TMI_BF16; strides in elements, p_sq >= Tk,
 * p_sbh >= Tq * p_sq, no alignment beyond the element size (every Tk >= 1 works).  No atomics, no workspace: two calls
 * are bit-identical.  TMI_ERR_INVALID for a NULL descriptor / probs / stats, a bad dtype or stride, q or k that
 * tmi_attn_fwd would refuse, mask_mode 2 without key_bias, and dropout_p > 0 (these are inference-time weights). */
int tmi_attn_probs(const tmi_attn_desc* d, void* probs, int32_t probs_dtype, int64_t p_sbh, int64_t p_sq, void* stream);

/* ------------------------------------------------------------------------------------
 * Token-to-frame alignment (inference): cross-attention weights -> a cost, and dynamic time warping over it.
 *
 * tmi_align_cost.  probs: one decoder layer's cross-attention weights, element (n, h, s, t) at
 * probs[(n*H + h)*p_sbh + s*p_sq + t], TMI_F32 or TMI_BF16, as tmi_attn_probs writes them (p_sq >= T, p_sbh >= S*p_sq;
 * the caller points past the start token's row).  rows[N], cols[N]: device int32, the tokens to align and the valid
 * encoder frames of item n, 1 <= rows[n] <= S, medfilt_width/2 < cols[n] <= T.  head_weight[H]: device fp32; a head
 * of weight 0 is skipped and its weights are never read.  medfilt_width: odd, 1..9 (1: no filter).  Per item n, head h
 * of non-zero weight and frame t < cols[n], in fp32:
 *   normalise  z[s,t] = (p[s,t] - mean[t]) * rsqrt(var[t] + 1e-20), mean and var over the rows s < rows[n] only, var the
 *              population variance (/ rows[n]) of the deviations from that mean (two passes), so rows[n] == 1 gives
 *              exactly 0; normalize == 0: z = p.
 *   filter     m[s,t] = the median of z[s, t - w/2 .. t + w/2], indices reflected about the ends of [0, cols[n]) without
 *              repeating the end sample (-k -> k, cols-1+k -> cols-1-k: numpy pad "reflect", scipy.ndimage "mirror").
 *              The median selects one of the z: it adds no rounding.
 *   combine    acc = accumulate ? cost[n,s,t] : 0;  for h ascending: acc = fma(-head_weight[h], m_h[s,t], acc);
 *              cost[n*c_sn + s*c_ss + t] = acc.
 * Elements with s >= rows[n] or t >= cols[n] are not written (c_ss >= T, c_sn >= S*c_ss); an item with rows[n] < 1 is
 * skipped by both kernels (nothing of it is read or written).  Several layers are folded
 * by successive calls with accumulate = 1 on one stream.  No atomics, no workspace: the same call gives the same bits.
 * tmi_align_cost_tile: the output frames of one workgroup for a width (64 - (w - 1)), -1 for a width that is refused.
 * TMI_ERR_INVALID: a NULL pointer, a bad dtype / width / flag / stride, N outside 1..65535, H outside 1..32, T <= w/2.
 *
 * tmi_dtw.  cost: element (n, i, j) at cost[n*c_sn + i*c_ss + j], fp32; rows, cols as above (cols[n] >= 1).  With
 * D[-1][-1] = 0 and every other border +inf,
 *   D[i][j] = cost[i][j] + min(c0 = D[i-1][j-1], c1 = D[i-1][j], c2 = D[i][j-1])                      (fp32)
 *   move    = 0 (diagonal) if c0 < c1 && c0 < c2, else 1 (up) if c1 < c0 && c1 < c2, else 2 (left)
 * so the first column moves up, the first row moves left, and a tie goes left - also the tie c0 == c1 < c2, in which
 * the path then leaves the minimum that D took.  The path is traced back from (rows-1, cols-1) to (0, 0).
 *   tok_start[n*S_max + i], tok_end[n*S_max + i]: the first frame of the path in row i, and its last frame + 1
 *   total[n] = D[rows-1][cols-1]
 *   path (may be NULL, then path_len too): int32 (i, j) pairs in forward order at path[(n*(S_max+T_max-1) + k)*2],
 *   k < path_len[n]
 * Entries at or past rows[n] / path_len[n] are not written.  One workgroup per item, one thread per row: S_max <= 1024,
 * T_max <= 4096, N <= 65535.  workspace: tmi_dtw_workspace_bytes (the moves, 2 bits per cell; -1 outside those
 * limits), any contents.  No atomics: the same call gives the same bits. */
int64_t tmi_align_cost_tile(int32_t medfilt_width);
int tmi_align_cost(const void* probs, int32_t probs_dtype, int64_t p_sbh, int64_t p_sq, const int32_t* rows,
                   const int32_t* cols, const float* head_weight, float* cost, int64_t c_sn, int64_t c_ss, int64_t N,
                   int64_t H, int64_t S, int64_t T, int32_t medfilt_width, int32_t normalize, int32_t accumulate,
                   void* stream);
int64_t tmi_dtw_workspace_bytes(int64_t N, int64_t S_max, int64_t T_max);
int tmi_dtw(const float* cost, int64_t c_sn, int64_t c_ss, const int32_t* rows, const int32_t* cols, int64_t N,
            int64_t S_max, int64_t T_max, int32_t* tok_start, int32_t* tok_end, float* total, int32_t* path,
            int32_t* path_len, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Error-rate evaluation: tmi_edit_distance, the batched Levenshtein distance with operation counts between token rows that
 * are already on the device (Whisper's generated sequences against labels, CTC transcripts against labels, n-best lists
 * against one reference).  Integers only: every output is exact.
 *
 * hyp int32, element (i, c) at hyp[i*hyp_ld + c], N rows of which the first hyp_cols columns are read; hyp_len int32 [N]
 * or NULL (every row is hyp_cols long).  ref int32, element (b, c) at ref[b*ref_ld + c], N / R rows, ref_cols columns
 * read; ref_len int32 [N / R] or NULL.  R >= 1 divides N: pair i is hypothesis i against reference i / R (the layout of
 * num_return_sequences).  out int32, pair i at out[i*out_ld .. i*out_ld + 6), out_ld >= 6.
 * Normalisation, of both sides alike, in the kernel:
 *   a row is its first min(len, cols) tokens (a negative len counts as 0);
 *   it is cut before the first occurrence of stop_id (stop_id == -1: no cut);
 *   every token x with skip_lo <= x < skip_hi is dropped (skip_lo >= skip_hi: none is).
 * A token is only compared, never used as an index: any int32 value, and anything past the length, is harmless.
 * The rule.  h[1..n], r[1..m] the kept tokens; a cell is the tuple (d, sub, del, ins):
 *   C[0][0] = (0, 0, 0, 0),  C[i][0] = (i, 0, 0, i),  C[0][j] = (j, 0, j, 0)
 *   C[i][j] = the first of these candidates whose d is smallest (a later one replaces an earlier one only when its d is
 *             strictly smaller):
 *               1. diagonal  C[i-1][j-1], with d + 1, sub + 1 when h[i] != r[j]
 *               2. up        C[i-1][j]    with d + 1, ins + 1   (a hypothesis token with no partner)
 *               3. left      C[i][j-1]    with d + 1, del + 1   (a reference token with no partner)
 *   out[i] = (d, sub, del, ins, n, m) of C[n][m]
 * so d is the Levenshtein distance, sub + del + ins == d and ins - del == n - m.
 * One workgroup per pair; both rows are compacted into LDS in order (a ballot over the keep flags), the table is swept by
 * anti-diagonals with three rotating diagonals of packed cells in LDS and one barrier per diagonal (csrc/edit.hip).
 * Limits: 0 <= hyp_cols, ref_cols <= 4096, 1 <= N <= 65535, hyp_ld >= hyp_cols, ref_ld >= ref_cols, strides <= 2^30.
 * TMI_ERR_INVALID, before anything is launched and with nothing written: hyp, ref or out NULL, a pointer that is not
 * 4-byte aligned, a size outside those limits, R < 1 or not dividing N, a stride too small.
 * No atomics, no workspace: the same call gives the same bits.
 * Not built: a backtrace - no per-token operations and no alignment come out, only the counts. */
int tmi_edit_distance(const int32_t* hyp, int64_t hyp_ld, int64_t hyp_cols, const int32_t* hyp_len, const int32_t* ref,
                      int64_t ref_ld, int64_t ref_cols, const int32_t* ref_len, int64_t N, int64_t R, int32_t stop_id,
                      int32_t skip_lo, int32_t skip_hi, int32_t* out, int64_t out_ld, void* stream);

/* tmi_edit_align: the same table, and the alignment itself.  The inputs, the normalisation, the rule, the limits and out
 * are those of tmi_edit_distance (out[i] holds the same six numbers as that call on the same arguments).  In addition
 * every cell with i >= 1 and j >= 1 records which candidate won - diagonal, up or left; row 0 moves left and column 0
 * moves up - and the path is traced from (n, m) to (0, 0).  The tie rule makes that path unique.
 *   n_steps[i]  the length of pair i's path, = m + ins = n + del
 *   steps       int32, element (i, k, f) at steps[i*steps_ld + 3*k + f], k < n_steps[i], in forward order (from the start
 *               of both rows):
 *     f = 0  the operation: 0 match, 1 substitution, 2 deletion (a reference token with no partner, a left move),
 *            3 insertion (a hypothesis token with no partner, an up move)
 *     f = 1  the hypothesis token's column in the caller's row as passed in - before the cut and before skipped tokens
 *            were dropped; -1 for a deletion
 *     f = 2  the reference token's column in the caller's row, likewise; -1 for an insertion
 * so hyp[i*hyp_ld + steps[..1]] and ref[(i/R)*ref_ld + steps[..2]] are the tokens a step names, and the same columns
 * index whatever else the caller keeps per token (timestamps, frames).  Entries at or past n_steps[i] are not written.
 * A pair with an empty side is m deletions, n insertions, or no step at all.  The numbers of steps with op 1, 2, 3 are
 * out[1], out[2], out[3].
 * steps_ld >= 3 (hyp_cols + ref_cols), <= 2^30.  workspace: tmi_edit_align_workspace_bytes (-1 outside the limits on N and
 * the columns), any contents; it holds the moves, two bits a cell, as the two 64-bit ballots of every 64 neighbouring
 * cells of an anti-diagonal: 16 (hyp_cols + ref_cols + 1) ((min(hyp_cols, ref_cols) + 64) / 64) bytes a pair (csrc/edit.hip
 * has the layout).  LDS: tmi_edit_distance's plus 2 (hyp_cols + ref_cols) bytes for the columns, 147480 at the limits.
 * TMI_ERR_INVALID, before anything is launched and with nothing written: what tmi_edit_distance refuses; steps, n_steps or
 * workspace NULL or not 4-byte aligned; steps_ld too small; workspace_bytes below the size function's value.
 * The sweep is parallel; the trace is one lane's walk of at most n + m steps.
 * No atomics, no allocation, no synchronisation: the same call gives the same bits.
 *
 * tmi_edit_confusion folds the steps of many pairs into a confusion table.  steps, steps_ld, n_steps as tmi_edit_align
 * wrote them, hyp / ref with the strides, columns, N and R of that call.  first_only = 1 counts only the pairs i with
 * i % R == 0.  1 <= V <= 1024.  counts int32 [(V + 1) (V + 1) + 1]: element (row, col) at counts[row*(V + 1) + col], the
 * row is the reference token and the column the hypothesis token of a step, index V stands for "none" - a deletion lands
 * in column V, an insertion in row V, a match on the diagonal.  This is the one place where a token becomes an index: a
 * step with a token outside [0, V) (or with an op or a column that tmi_edit_align cannot have written) is not indexed
 * but counted in the trailing element counts[(V + 1) (V + 1)].  accumulate = 0 zeroes counts first, 1 adds to what it
 * holds.  One workgroup per pair, one global integer atomic add per step: integer adds commute, so the same call gives
 * the same bits.  TMI_ERR_INVALID: a NULL or misaligned pointer, sizes or strides that tmi_edit_align refuses, V outside
 * 1..1024, a flag that is not 0 or 1.
 * Not built: text normalisation (case, punctuation, numerals), and mapping an error to a time - the columns index the
 * caller's per-token times directly. */
int64_t tmi_edit_align_workspace_bytes(int64_t N, int64_t hyp_cols, int64_t ref_cols);
int tmi_edit_align(const int32_t* hyp, int64_t hyp_ld, int64_t hyp_cols, const int32_t* hyp_len, const int32_t* ref,
                   int64_t ref_ld, int64_t ref_cols, const int32_t* ref_len, int64_t N, int64_t R, int32_t stop_id,
                   int32_t skip_lo, int32_t skip_hi, int32_t* out, int64_t out_ld, int32_t* steps, int64_t steps_ld,
                   int32_t* n_steps, void* workspace, int64_t workspace_bytes, void* stream);
int tmi_edit_confusion(const int32_t* steps, int64_t steps_ld, const int32_t* n_steps, const int32_t* hyp, int64_t hyp_ld,
                       int64_t hyp_cols, const int32_t* ref, int64_t ref_ld, int64_t ref_cols, int64_t N, int64_t R,
                       int32_t first_only, int64_t V, int32_t* counts, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * CTC inference (wav2vec2.py Wav2Vec2ForCTC: V:940-1001, forward only): the head's log-softmax, the greedy collapse, the
 * loss and the forced alignment.  All arithmetic is fp32; `blank` is an argument; -inf is the additive zero, and a
 * log-sum-exp LSE whose inputs are all -inf is -inf, never NaN.  No atomics, no allocation, no synchronisation: the same
 * call gives the same bits.  Values in device memory (labels, lengths, argmaxes) are not seen by the calls: a length is
 * clamped to its tensor, a symbol outside [0, lp_st) resp. [0, lp_ld) is never dereferenced.
 *
 * tmi_ctc_logsoftmax.  logits fp32, element (r, c) at logits[r*ld + c]; per row r < R over the columns c < V:
 *   m = max x,  lse = m + log(sum exp(x - m)),  logp[r*lp_ld + c] = x[c] - lse,
 *   argmax[r] = the smallest column among equal maxima of the given logits (a comparison of fp32 values: exact).
 * 2 <= V <= 64 (one lane per column), ld >= V, lp_ld >= V, R <= 2^30.  Columns past V and rows past R are neither read
 * nor written.  A row that is -inf throughout gives NaN.
 *
 * tmi_ctc_greedy.  argmax int32 [N][T_max], logp fp32 [N][T_max][lp_ld], frame_lens int32 [N].  With a = argmax of item n
 * and len = min(frame_lens[n], T_max): frame t < len emits its token when a[t] != blank && (t == 0 || a[t] != a[t-1]).
 *   tokens[n*T_max + k]    the k-th emitted token, in frame order, dense
 *   tok_start[n*T_max + k] that frame;  tok_end[n*T_max + k] the last frame of its run of equal argmaxes, plus 1
 *   out_len[n]             the number of emitted tokens
 *   best_logprob[n]        sum over t < len of logp[t][a[t]]: thread i of 256 adds its frames t = i, i + 256, .. in
 *                          ascending t, the 64 lanes of a wave meet in a butterfly (lane distance 32, 16, .., 1), the four
 *                          wave sums are added ((w0 + w1) + w2) + w3
 * Entries at or past out_len[n] are not written; an item with frame_lens[n] < 1 is skipped entirely (nothing of it is
 * read or written, out_len[n] included).  1 <= N <= 65535 (one workgroup each), T_max, lp_ld <= 2^30.
 *
 * tmi_ctc_forward.  logp: element (n, t, c) at logp[n*lp_sn + t*lp_st + c]; labels int32 [N][L_max]; L = label_lens[n],
 * T = frame_lens[n]; ext = [blank, l1, blank, l2, .., blank] with S = 2L + 1 states:
 *   alpha_0(0) = lp[0][blank], alpha_0(1) = lp[0][l1], every other -inf
 *   alpha_t(s) = lp[t][ext_s] + LSE(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2))
 *                the third term only if ext_s != blank && ext_s != ext_{s-2}
 *   LSE(a0, a1, a2) = m + log((exp(a0 - m) + exp(a1 - m)) + exp(a2 - m)), m = the maximum, an absent term -inf
 *   nll[n] = -LSE(alpha_{T-1}(S-1), alpha_{T-1}(S-2));  L = 0: -alpha_{T-1}(0)
 * An item without a path (too few frames, T < 1) gives nll = +inf and infeasible[n] = 1 (else 0); with zero_infinity its
 * nll is 0.  One workgroup per item, one thread per extended state: 1 <= L_max <= 511, 1 <= N <= 65535,
 * 1 <= T_max <= 2^31 - 17, lp_sn >= T_max*lp_st, 0 <= blank < lp_st <= 2^30.
 *
 * tmi_ctc_viterbi.  The same recursion with max for LSE: the candidates are compared in the order stay (s), step (s-1),
 * skip (s-2), the largest wins and a tie goes to the earliest in that order.  The end state is S-2 if its value is
 * strictly larger than that of S-1, else S-1.  The path is traced back on the device:
 *   tok_start[n*L_max + i] the first frame in state 2i + 1, tok_end[n*L_max + i] the last such frame plus 1  (i < L)
 *   total[n]               the path's log-probability
 *   states (may be NULL)   int32 [N][T_max]: the extended state of frame t < T
 * An item without a path: total = -inf, bounds -1, states -1, infeasible[n] = 1.  Nothing past label_lens[n] or
 * frame_lens[n] is written.  T_max <= 4096 here; workspace: tmi_ctc_workspace_bytes (the moves, 2 bits per frame and
 * state; -1 outside the limits), any contents.
 * TMI_ERR_INVALID (nothing is launched): a NULL or misaligned pointer, a size outside the limits above, a stride too
 * small, blank outside the row, a flag that is not 0 / 1, a workspace too small. */
int tmi_ctc_logsoftmax(const float* logits, int64_t ld, int64_t R, int64_t V, float* logp, int64_t lp_ld, int32_t* argmax,
                       void* stream);
int tmi_ctc_greedy(const int32_t* argmax, const float* logp, int64_t lp_ld, const int32_t* frame_lens, int32_t blank,
                   int32_t* tokens, int32_t* out_len, int32_t* tok_start, int32_t* tok_end, float* best_logprob, int64_t N,
                   int64_t T_max, void* stream);
int tmi_ctc_forward(const float* logp, int64_t lp_sn, int64_t lp_st, const int32_t* labels, const int32_t* label_lens,
                    const int32_t* frame_lens, int32_t blank, float* nll, int32_t* infeasible, int64_t N, int64_t L_max,
                    int64_t T_max, int32_t zero_infinity, void* stream);
int64_t tmi_ctc_workspace_bytes(int64_t N, int64_t L_max, int64_t T_max);
int tmi_ctc_viterbi(const float* logp, int64_t lp_sn, int64_t lp_st, const int32_t* labels, const int32_t* label_lens,
                    const int32_t* frame_lens, int32_t blank, int32_t* tok_start, int32_t* tok_end, float* total,
                    int32_t* states, int32_t* infeasible, int64_t N, int64_t L_max, int64_t T_max, void* workspace,
                    int64_t workspace_bytes, void* stream);

/* tmi_ctc_posteriors (csrc/ctc_post.hip).  The forward-backward pass over the same lattice: alpha as tmi_ctc_forward, beta
 * its mirror, and what the two give together.  fp32 throughout, -inf the additive zero, LSE3 exactly the LSE of
 * tmi_ctc_forward, no atomics, no scratch besides gamma.  logp, labels, label_lens, frame_lens, blank as tmi_ctc_forward,
 * with V columns; ext = [blank, l1, blank, .., lL, blank], S = 2L + 1, T = min(frame_lens[n], T_max), lp = logp[n].
 *   alpha:  alpha_t(s) is the recursion of tmi_ctc_forward, in the same operation order.  nll[n] and infeasible[n] are bit
 *           for bit what tmi_ctc_forward writes for the same arguments, zero_infinity included.  ll = -(the unclamped nll).
 *   beta:   beta_{T-1}(s) = lp[T-1][ext_s] for s = S-1 and, if S > 1, s = S-2; -inf elsewhere.
 *           beta_t(s) = lp[t][ext_s] + LSE3(beta_{t+1}(s), beta_{t+1}(s+1), beta_{t+1}(s+2)).
 *           The second term applies only if s+1 < S.
 *           The third term applies only if s+2 < S && ext_{s+2} != blank && ext_{s+2} != ext_s.
 *   gamma:  gamma[n,t,s] = exp((alpha_t(s) - ll) + (beta_t(s) - lp[t][ext_s])): the two differences first, then their sum.
 *           It is 0 whenever alpha_t(s) or beta_t(s) is -inf.  gamma is not clamped to 1.
 *           Element (n, t, s) at gamma[(n*T_max + t)*(2*L_max + 1) + s]; the tensor is the call's scratch for alpha first.
 *   occ:    occ[n,t,c] = sum over s ascending with ext_s == c of gamma[n,t,s], a running sum from 0.  The value is 0 for
 *           a symbol that is not in ext.  Element (n, t, c) at occ[n*oc_sn + t*oc_st + c].
 *   grad (may be NULL):  grad[n,t,c] = expf(lp[t][c]) - occ[n,t,c], at grad[n*gr_sn + t*gr_st + c].  This is
 *           d nll[n] / d logits[n,t,c] for logits whose row-wise log-softmax is lp; per item and unscaled ("sum").
 *   tok_frames:  tok_frames[n*L_max + i] = sum over t of gamma[n,t,2i+1], a running sum from 0 in descending t
 *           (t = T-1, T-2, .., 0: the order of the beta pass).
 *   tok_center:  tok_center[n*L_max + i] = (sum over t of t * gamma[n,t,2i+1]) / tok_frames[n,i], in frames.  The product
 *           t * gamma is formed with t converted to fp32 and rounded before it is added.  The sum takes the same order as
 *           tok_frames.
 *   Written: gamma for t < T, s < S; occ / grad rows t < T, columns c < V; tok_* for i < L.  Everything else is left
 *   untouched: rows past the clip, columns past V, states past S, tokens past L.
 *   An item without a path (T < 1, or no finite path): nll / infeasible as tmi_ctc_forward; every gamma / occ / grad
 *   element listed above is 0; tok_frames = 0, tok_center = -1.  With T < 1 only the tok_* entries exist.
 * The same call gives the same bits; an item in a ragged batch gets the bits it gets alone.  A label length is clamped to
 * [0, L_max], a frame length to T_max, and a symbol outside [0, V) is never dereferenced: its log-prob is -inf.
 * 1 <= N <= 65535, 1 <= L_max <= 511, 1 <= T_max <= 4096, 2 <= V <= 64, 0 <= blank < V, V <= lp_st <= 2^30,
 * lp_sn >= T_max*lp_st, and the same for oc_st / oc_sn and (grad given) gr_st / gr_sn; 4-byte aligned non-NULL pointers,
 * grad excepted; zero_infinity 0 / 1.  Anything else: TMI_ERR_INVALID, nothing is launched. */
int tmi_ctc_posteriors(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* labels,
                       const int32_t* label_lens, const int32_t* frame_lens, int32_t blank, float* nll, int32_t* infeasible,
                       float* gamma, float* occ, int64_t oc_sn, int64_t oc_st, float* grad, int64_t gr_sn, int64_t gr_st,
                       float* tok_frames, float* tok_center, int64_t N, int64_t L_max, int64_t T_max, int32_t zero_infinity,
                       void* stream);

/* tmi_ctc_beam.  CTC prefix beam search over logp (element (n, t, c) at logp[n*lp_sn + t*lp_st + c], c < V), fp32
 * throughout, -inf the additive zero, no atomics: the same call gives the same bits, and an item's results do not depend
 * on the other items of the call.  LSE2(a, b) = m + log(exp(a - m) + exp(b - m)) with m = max(a, b), -inf when m is.
 *   State.  A beam is a prefix y (non-blank tokens, possibly none) with pb (its paths that end in a blank) and pnb (those
 *   that end in its last token e).  The start: one beam, y = (), pb = 0, pnb = -inf.  Beams are kept by descending score.
 *   Frame t < T = min(frame_lens[n], T_max), lp = logp[n, t, :], for beam k of the current set, tot = LSE2(pb, pnb):
 *     stay (candidate index k):          pb' = lp[blank] + tot;  pnb' = lp[e] + pnb, -inf for the empty prefix
 *     extension by c != blank (index K + k*V + c):  v = lp[c] + (c == e ? pb : tot)
 *       if the sequence y + c is itself a beam p of the current set, v is folded into p's stay candidate,
 *       pnb'_p = LSE2(pnb'_p, v), and the extension is no candidate of its own (one extension at most folds into a beam);
 *       otherwise it is a candidate with pb' = -inf, pnb' = v
 *     a candidate's score is LSE2(pb', pnb') - for a pure extension v itself.  The next set: the up to K candidates of
 *     largest finite score, among equal scores the lower candidate index first; a candidate whose score is -inf is never
 *     kept, so a set may hold fewer than K beams (or none).
 *   "Is a beam of the current set" is equality of the token sequences: a prefix that fell out of the set and was created
 *   again is the same prefix (a hash filters, a walk of the two chains confirms).
 *   tokens int32 [N][K][T_max]  rank r's sequence, dense, in frame order; nothing is written past its length
 *   lengths int32 [N][K], scores fp32 [N][K]  the final LSE2(pb, pnb), descending; n_beams int32 [N]  the ranks filled;
 *   a rank past it has length 0 and score -inf.  An item with T < 1 returns the start state: one empty beam, score 0.
 * One workgroup per item, one wave per beam, one lane per symbol: 1 <= K <= 16, 2 <= V <= 64, V <= lp_st <= 2^30,
 * lp_sn >= T_max*lp_st, 0 <= blank < V, 1 <= N <= 65535, 1 <= T_max <= 65536.  workspace: tmi_ctc_beam_workspace_bytes
 * (the prefix trie, one (parent node, token) record per frame and rank; -1 outside the limits), 8-byte aligned, any
 * contents.  Values in device memory are not trusted: a length is clamped to T_max, and no symbol is read from memory
 * that this call did not write.  TMI_ERR_INVALID (nothing is launched): a NULL or misaligned pointer, a size outside
 * the limits, a stride too small, blank outside the row, a workspace too small. */
int64_t tmi_ctc_beam_workspace_bytes(int64_t N, int64_t K, int64_t T_max);
int tmi_ctc_beam(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* frame_lens, int32_t blank,
                 int32_t K, int32_t* tokens, int32_t* lengths, float* scores, int32_t* n_beams, int64_t N, int64_t T_max,
                 void* workspace, int64_t workspace_bytes, void* stream);

/* tmi_ctc_beam_lm.  tmi_ctc_beam with an n-gram language model and a length bonus in the ranking, applied while the search
 * runs (shallow fusion): everything above holds - pb, pnb, the fold, the tie rule, the limits, the workspace - and this:
 *   The table.  lm fp32, dense, row-major, V^lm_order entries, 1 <= lm_order <= 4, V^lm_order <= 2^24.  lm[ctx*V + c] is
 *   log P(c | the previous lm_order - 1 tokens); ctx reads those tokens as base-V digits, the most recent one last.  A
 *   context slot before the start of the sequence holds `blank` (never a token, so its index is free to mean "nothing
 *   yet"): the start context is blank*(1 + V + ... + V^(lm_order-2)), and after an extension by c
 *   ctx' = (ctx*V + c) mod V^(lm_order-1) - always 0 for lm_order 1.  Column `blank` is never read, nor a row with a blank
 *   behind a non-blank.  Entries are finite or -inf; a -inf entry is a forbidden transition: that extension is no
 *   candidate and is not folded.
 *   The beam state.  Every beam carries g in fp32, 0 at the start state.  An extension of beam k by c gets
 *   g' = g_k + fmaf(lm_alpha, lm[ctx_k*V + c], lm_beta) (one fma, one add; lm_alpha >= 0, both weights finite); a stay
 *   candidate keeps g_k.  The fold adds CTC mass only: g is a function of the token sequence alone, computed by the same
 *   operations in the same order whichever parent created the beam, so the beam that is folded into already holds
 *   exactly the g the extension would have got.
 *   Ranking.  A candidate ranks by LSE2(pb', pnb') + g (one fp32 add) where tmi_ctc_beam ranks by LSE2(pb', pnb'); a
 *   candidate whose CTC score is -inf is never kept.
 *   scores fp32 [N][K]  the final LSE2(pb, pnb) + g, descending; ctc_scores [N][K]  LSE2(pb, pnb); lm_scores [N][K]  g.
 *   A rank past n_beams holds -inf, -inf and 0.
 * Not built: an end-of-sequence term, word-level models, lexicons beyond -inf entries, backoff structures.
 * TMI_ERR_INVALID (nothing is launched): what tmi_ctc_beam refuses; lm, ctc_scores or lm_scores NULL or not 4-byte
 * aligned; lm_order outside 1..4; V^lm_order > 2^24; lm_alpha negative or not finite; lm_beta not finite.  The table's
 * values are not checked on the device (Wav2Vec2's check_ctc_lm_args does it on the host). */
int tmi_ctc_beam_lm(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* frame_lens, int32_t blank,
                    int32_t K, const float* lm, int32_t lm_order, float lm_alpha, float lm_beta, int32_t* tokens,
                    int32_t* lengths, float* scores, float* ctc_scores, float* lm_scores, int32_t* n_beams, int64_t N,
                    int64_t T_max, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Decoder token embedding + positional encoding (W:405-408) with the teacher-forcing
 * shift of W:559-563 folded in: id(b,t) = t == 0 ? start_id : labels[b, t-1].
 *   out[b,t,:] = table[id(b,t), :] + pe[t, :]
 * Backward (gradient of tf.gather, densified): for every distinct id, dtable[id,:] =
 * sum over its positions of dy, summed in position order (deterministic, no atomics).
 * dtable must be zero on entry for rows that are not touched.
 */
int tmi_embed_fwd(const int32_t* labels, const float* table, const float* pe, void* out,
                  int64_t B, int64_t S, int64_t D, int32_t start_id, int32_t dtype, void* stream);
int tmi_embed_bwd(const int32_t* labels, const void* dy, float* dtable, int64_t B, int64_t S,
                  int64_t D, int32_t start_id, int32_t dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * Shifted sparse softmax cross-entropy over logits[B*S, ld] (W:585-600):
 * row (b,t) with t < S-1 is scored against labels[b, t+1]; row t = S-1 is unused.
 *   row_loss[b*S+t] = logsumexp(logits) - logits[target]      (0 for unused rows)
 *   logits <- dlogits = (softmax - onehot) * grad_scale       (0 for unused rows and for
 *                                                              the pad columns [V, ld))
 * grad_scale is 1 / (B*(S-1)) for the reference's reduce_mean.  tmi_mean_rows folds
 * row_loss into loss[0] = sum(row_loss) * scale.
 * The pad columns [V, ld) and the unused rows are masked by index and never enter the result: on entry they may hold
 * anything, NaN included (as for tmi_logprob_fold); on return they are +0.
 */
int tmi_xent_fwd_bwd(void* logits, int64_t ld, const int32_t* labels, float* row_loss,
                     int64_t B, int64_t S, int64_t V, float grad_scale, int32_t dtype, void* stream);
/* The same cross-entropy for logits that are the output of an LM head (W:579-600: logits = decoder_out . lm_head): x[B*S, d]
 * (row stride x_ld) and w (element (k, n) at w[k*w_sk + n*w_sn]) are the operands tmi_gemm produced `logits` from.  bf16
 * logits have lost the low bits of the target logit (ulp 0.03 at |z| in [4, 8)) and the loss is lse - z_target, so the row's
 * workgroup recomputes z_target = x[row, :] . w[:, target] in fp32 for row_loss; lse and the gradient come from `logits` as
 * in tmi_xent_fwd_bwd.  On the headline golden this takes the bf16 loss-curve error from 7.7e-4 to 2.0e-4
 * (profiles/r04_bf16_margin.txt).  fp32 logits: identical to tmi_xent_fwd_bwd (x, w are validated and ignored). */
int tmi_linear_xent(const void* x, int64_t x_ld, const void* w, int64_t w_sk, int64_t w_sn, int64_t d, void* logits, int64_t ld,
                    const int32_t* labels, float* row_loss, int64_t B, int64_t S, int64_t V, float grad_scale, int32_t dtype,
                    void* stream);
int tmi_sum_scale(const float* x, float* out, int64_t n, float scale, void* stream);

/* ------------------------------------------------------------------------------------
 * The weighted loss of W:596-598 (a decoder_attention_mask was given):
 *   loss = sum(nll * mask[:, :-1]) / sum(mask[:, :-1])
 * on the training path.  The normaliser is a sum over the mask, which lives in device memory: it is taken on the device and
 * handed from kernel to kernel there (inv_wsum), so the step never reads it on the host and a recorded launch plan replays
 * unchanged for every mask.
 *
 * tmi_xent_weights: the row weights of a [B, S] fp32 mask (row stride mask_ld) and their normaliser, one workgroup:
 *   row_w[b*S+t] = max(mask[b, t], 0) for t < S-1, and 0 for t = S-1 (W:597 slices the last column off: it is never read);
 *                  an entry that is not > 0 (negative, NaN) counts as 0
 *   wsum         = sum(row_w), in fp32 in a fixed order (tmi_sum_scale's): bit-reproducible, exact for 0/1 masks
 *   inv_wsum[0]  = 1.0f / wsum if wsum > 0, else 0
 * wsum == 0 (every weight 0): the reference would divide 0 by 0; here the batch then contributes loss 0 and all-zero
 * gradients, as a replica whose slice of the batch is empty does.
 *
 * tmi_xent_weighted / tmi_linear_xent_weighted: tmi_xent_fwd_bwd / tmi_linear_xent with a weight per row.
 *   scored row   (row_w[r] > 0): the unweighted arithmetic, unchanged in each of the three kernels, with
 *                grad_scale = loss_scale * row_w[r] * inv_wsum[0] (in this order) and row_loss[r] = row_w[r] * nll.  With an
 *                all-ones mask and loss_scale = 1 that is fl(1 / (B*(S-1))), the scalar the unweighted call is given: the
 *                results are bit-identical.
 *   unscored row (row_w[r] == 0, and every row t = S-1): the row of logits is NOT read; its gradient is +0 over all ld
 *                columns and row_loss[r] = 0, whatever the row held, non-finite values included (TensorFlow's inf * 0 is
 *                NaN; this is a defined departure, and the only work the mask saves: the LM-head GEMMs still run over all
 *                rows).
 * The loss is tmi_sum_scale_dev(row_loss, loss, B*S, inv_wsum): out[0] = sum(x[0..n)) * scale[0], tmi_sum_scale with the
 * scale read from device memory.  None of the four takes an argument that changes from step to step. */
int tmi_xent_weights(const float* mask, int64_t mask_ld, int64_t B, int64_t S, float* row_w, float* inv_wsum, void* stream);
int tmi_xent_weighted(void* logits, int64_t ld, const int32_t* labels, const float* row_w, const float* inv_wsum,
                      float* row_loss, int64_t B, int64_t S, int64_t V, float loss_scale, int32_t dtype, void* stream);
int tmi_linear_xent_weighted(const void* x, int64_t x_ld, const void* w, int64_t w_sk, int64_t w_sn, int64_t d, void* logits,
                             int64_t ld, const int32_t* labels, const float* row_w, const float* inv_wsum, float* row_loss,
                             int64_t B, int64_t S, int64_t V, float loss_scale, int32_t dtype, void* stream);
int tmi_sum_scale_dev(const float* x, float* out, int64_t n, const float* scale, void* stream);

/* ------------------------------------------------------------------------------------
 * Greedy decoding's next token (W:675 / W:697: argmax(lm_head(decoder_out)[:, -1, :]), with the final decoder LayerNorm of
 * W:466 in front): for each of M hidden-state rows x[r * x_ld + k] (k < d; fp32 or bf16: x_dtype)
 *   y    = gamma, beta given ? LayerNorm_eps(x[r, :]) (fp32 statistics, W:392) : x[r, :]
 *   z[n] = sum_k y[k] * w[k * w_ld + n]        (w: the LM head in its stored [d, w_ld] layout, fp32 or bf16: w_dtype;
 *                                              fp32 accumulation, in a fixed order: bit-reproducible)
 *   ids[r * ids_ld] = argmax_{n < V} z[n]       (int32; the smallest n among equal maxima, as tf.argmax; -0 == +0;
 *                                              the pad columns [V, w_ld) are never chosen)
 *   eos_count[0] = #{r : ids[r * ids_ld] == eos_id}   (int32; eos_id < 0: 0; eos_count may be NULL)
 * x_ld is an arbitrary row stride (the last position of each sample, read in place).  gamma and beta are both given or
 * both NULL.  w must be 16-byte aligned, w_ld a multiple of 8 and >= V.  One launch: the weights are streamed once
 * (for M <= 16; M rows in groups of 16 otherwise); the workgroups' candidates meet in `workspace` (>= 8 * (M + 1) bytes,
 * 8-byte aligned, ZERO before the first call: the launch leaves it zero again, so one buffer serves every step on one
 * stream; concurrent calls need one each).  d * min(M, 16) * 4 bytes of LDS must fit in 160 KiB (d <= 2544 at M >= 16).
 */
int tmi_lm_head_argmax(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, float eps,
                       const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V, int32_t* ids,
                       int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace, int64_t workspace_bytes,
                       void* stream);

/* ------------------------------------------------------------------------------------
 * Beam search's next candidates (whisper.py generate, num_beams > 1): tmi_lm_head_argmax's LayerNorm and LM head, then
 * per row r of the M rows
 *   s[n] = z[n] * inv_temperature                     (n < V; the pad columns [V, w_ld) are never chosen)
 *   lse[r] = log sum_{n < V} exp(s[n])               (fp32; the per-workgroup (max, sum) partials are folded in a fixed
 *                                                     order, not in arrival order: bit-reproducible; lse may be NULL)
 *   ids[r * N + j], logprobs[r * N + j], j < N       (the N largest s, ordered by s desc then column asc - ties go to the
 *                                                     smaller column, -0 == +0; logprobs = s - lse[r], fp32)
 * 1 <= N <= 16, N <= V <= 65536; inv_temperature finite and > 0.  x, gamma/beta and w as for tmi_lm_head_argmax (the
 * weights are streamed once per 16 rows, the logits never reach memory).  `workspace`: >= 8 * M * (1 + ceil(V / 128) *
 * (N + 1)) bytes, 8-byte aligned, ZERO before the first call; the last workgroup of each 16-row tile leaves its part zero again,
 * so one buffer serves every step on one stream (concurrent calls need one each).  LDS: max(d * MT, 4 * MT * 128, 2048)
 * floats, MT = M rounded up to a power of two, at most 16, must fit in 160 KiB - 256 bytes (d <= 2544 at M > 8).
 */
int tmi_lm_head_topk(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, float eps,
                     const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V, float inv_temperature,
                     int64_t N, int32_t* ids, float* logprobs, float* lse, void* workspace, int64_t workspace_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------
 * Sampled decoding's next token (whisper.py generate, do_sample): tmi_lm_head_argmax's LayerNorm and LM head, then per
 * row r of the M rows
 *   s[n]  = z[n] / temperature  (n < V),  s[suppress_id] = -inf    (suppress_id -1: none)
 *   lse   = log sum_n exp(s[n])                                    (tmi_lm_head_topk's fixed-order fold)
 *   rk    = the dropout generator's row key of (stream key of seed and stream 0, row r), csrc/tmi_common.h;
 *   bits(c) = mix32(rk.a ^ mix32(c ^ rk.b))                        (mix32: the "lowbias32" finaliser)
 *   u(c)  = ((bits(c) >> 8) + 0.5) * 2^-24                          (never 0 or 1)
 * top_k == 0 (top_p must be 1): Gumbel-max over the vocabulary,
 *   token = argmax_n (s[n] - log(-log(u(n))))                      (fp32; ties: the smaller column)
 * 1 <= top_k <= 64: candidates c_0 .. c_{k-1} = the k largest z (ties: the smaller column first; every column that can
 *   be drawn when there are fewer than top_k), p_i = exp(s[c_i] - lse), P_j = p_0 + .. + p_j (fp32, in index order),
 *   m = the smallest m >= 1 with P_{m-1} >= top_p * P_{k-1} (top_p == 1: m = k),
 *   token = c_j for the smallest j < m with P_j > u(0xFFFFFFFF) * P_{m-1}, else c_{m-1}.
 *   top_k == 1 is exactly tmi_lm_head_argmax's token.  Ranking on z instead of s is deliberate: s = z / temperature
 *   is monotone in z, so the two orders differ only where two different z round to one fp32 s, and there the larger z
 *   goes first (not the smaller column): the finer order, and the one that makes top_k == 1 greedy at every temperature.
 * A row in which no column can be drawn (V == 1 and that column suppressed) writes pad_id and logprob 0.
 * ids[r * ids_ld] = token, logprob[r] = s[token] - lse (the unfiltered tempered distribution; logprob may be NULL).
 * finished[M] (int32, in and out): a row with finished[r] != 0 writes pad_id and logprob 0; a row that draws eos_id sets
 * finished[r] = 1.  n_finished[0] = the number of nonzero finished[] after the call.  The result does not depend on the
 * order in which workgroups finish.  temperature finite and > 0; 0 < top_p <= 1; V <= 65536; x, gamma/beta, w and the
 * LDS bound as for tmi_lm_head_topk.  `workspace`: >= tmi_lm_head_sample_workspace_bytes(M, V, top_k) bytes (-1 for
 * sizes the kernel refuses), 8-byte aligned, ZERO before the first call and left zero by every call.
 */
int64_t tmi_lm_head_sample_workspace_bytes(int64_t M, int64_t V, int64_t top_k);
int tmi_lm_head_sample(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, float eps,
                       const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V, float temperature,
                       int64_t top_k, float top_p, uint64_t seed, int32_t suppress_id, int32_t eos_id, int32_t pad_id,
                       int32_t* finished, int32_t* ids, int64_t ids_ld, float* logprob, int32_t* n_finished,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Decode constraints (whisper.py generate: repetition_penalty, no_repeat_ngram_size, suppress_tokens,
 * begin_suppress_tokens): per decoded row r two bit sets over the vocabulary, arrays of uint32 words, W = ceil(V / 32)
 * words a row at row stride bits_ld >= W; column n is bit n & 31 of word n >> 5.
 *   seen[r]:   the tokens the penalty applies to;     banned[r]: the tokens the row cannot emit.
 * With z[n] the LM-head logit exactly as tmi_lm_head_argmax / _topk / _sample compute it, for n < V
 *   z'[n] = -inf                         if banned bit n
 *         = z[n] / penalty  (z[n] > 0)   if seen bit n      (fp32, correctly rounded)
 *         = z[n] * penalty  (z[n] <= 0)  if seen bit n
 *         = z[n]                         otherwise
 * and the _c entry points are the originals' rules with z' in place of z - in every mode the edit comes BEFORE the
 * temperature: tmi_lm_head_argmax_c is argmax z' (same tie rule); tmi_lm_head_topk_c has s = z' * inv_temperature; in
 * tmi_lm_head_sample_c s = z' / temperature, suppress_id is one more ban and the candidates are ranked on z'.  The
 * logsumexp runs over the columns that are not banned; a banned column's log-probability is -inf and it is never drawn.
 * A row whose every column is banned: argmax writes column 0; top-k writes columns 0 .. N-1 with log-probability -inf
 * and lse -inf (never NaN); sample writes pad_id with log-probability 0.
 * The _c entry points take the originals' arguments and then seen, banned (either may be NULL: an empty set; other-
 * wise 4-byte aligned), bits_ld and penalty (finite, > 0; 1: none).  With both sets NULL the call IS the original (the
 * same kernel, the same bits).  Workspaces: the originals', same sizes, left zero - an original and its _c form can
 * alternate on one workspace.
 *
 * tmi_decode_constraints builds both sets for M rows from the rows' prefixes, one launch per decoding step:
 *   prefix [M, ld] int32, columns [0, t) of each row are read (1 <= t <= ld) and nothing past them;
 *   seen[r]   = { prefix[r, j] : j < t };
 *   banned[r] = static_banned (W words, the same for every row; NULL: empty)
 *               + { prefix[r, j + ngram - 1] : ngram >= 1, j + ngram - 1 <= t - 1,
 *                   prefix[r, j : j + ngram - 1] == prefix[r, t - ngram + 1 : t] }
 *     - the tokens that would complete an n-gram the prefix already holds; ngram 1: every token seen; ngram 0: none;
 *     nothing while t < ngram - 1.
 * A token id outside [0, V) is never used as an index and sets no bit.  All W words of both rows are written (the caller
 * never clears them), bits at or above V in the last word are 0, words [W, bits_ld) are left untouched.  The result is
 * the same bits in every run.  M <= 65535, V <= 65536, t <= 65536, ngram >= 0; anything else is TMI_ERR_INVALID and
 * launches nothing.
 */
int tmi_decode_constraints(const int32_t* prefix, int64_t ld, int64_t M, int64_t t, int64_t V,
                           const uint32_t* static_banned, int64_t ngram, uint32_t* seen, uint32_t* banned, int64_t bits_ld,
                           void* stream);
int tmi_lm_head_argmax_c(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, float eps,
                         const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V, int32_t* ids,
                         int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace, int64_t workspace_bytes,
                         const uint32_t* seen, const uint32_t* banned, int64_t bits_ld, float penalty, void* stream);
int tmi_lm_head_topk_c(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, float eps,
                       const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V, float inv_temperature,
                       int64_t N, int32_t* ids, float* logprobs, float* lse, void* workspace, int64_t workspace_bytes,
                       const uint32_t* seen, const uint32_t* banned, int64_t bits_ld, float penalty, void* stream);
int tmi_lm_head_sample_c(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, float eps,
                         const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V, float temperature,
                         int64_t top_k, float top_p, uint64_t seed, int32_t suppress_id, int32_t eos_id, int32_t pad_id,
                         int32_t* finished, int32_t* ids, int64_t ids_ld, float* logprob, int32_t* n_finished,
                         void* workspace, int64_t workspace_bytes, const uint32_t* seen, const uint32_t* banned,
                         int64_t bits_ld, float penalty, void* stream);

/* ------------------------------------------------------------------------------------
 * Timestamp rules (whisper.py generate, segment_timestamps): Whisper's timestamp tokens are the ids [tb, V), id tb + u
 * standing for u * 0.02 s, and a row is decoded under the grammar  <|t0|> text <|t1|><|t1|> text <|t2|> ..  The grammar is
 * more bans, OR-ed into the banned set of "Decode constraints" AFTER tmi_decode_constraints wrote it and before the step's
 * _c LM head reads it: two launches per step, tmi_timestamp_rules (rules a - f) then tmi_lm_head_timestamp_gate (rule g).
 * The row's generated tokens are g[0..n) = prefix[r, 1 + P : t], n = t - 1 - P (behind the start token and the P prompt
 * tokens).  isT(x): tb <= x < V (an id outside [0, V) is no timestamp and is never used as an index); "below": the
 * columns [0, tb), EOS and the specials among them.
 *   last = n >= 1 && isT(g[n-1]);   pen = n < 2 || isT(g[n-2]);   tl = the last g[j] with isT, or none.
 *   a. no_timestamps_id (>= 0) and every timestamp id > tb + max_ts are banned, always.
 *   b. n == 0: every below column is banned (EOS too), and every timestamp id > tb + max_initial (max_initial < 0: no cap).
 *   c. last && pen: every timestamp id is banned (after an opening timestamp or a closing/opening pair: text or EOS).
 *   d. last && !pen: every below column except eos_id is banned (after a closing timestamp: a timestamp or EOS).
 *   e. tl exists, last && !pen: the timestamp ids < tl are banned (the next segment may open where this one closed).
 *   f. tl exists, otherwise: the timestamp ids <= tl are banned.
 *   g. with z' the logit of "Decode constraints" under the set after a - f (so before the temperature),
 *        lse_ts = log sum exp z' over the timestamp columns not banned, max_below = max z' over the below columns not banned;
 *        lse_ts > max_below (fp32, strict; -inf on both sides is false, never NaN): every below column is banned.
 *
 * tmi_timestamp_rules: a - f for M rows in one launch.  prefix [M, ld] int32, columns [0, t) read (1 + P <= t <= ld);
 * banned [M, bits_ld] is read and written: bits are only added, only bits < V, a word with nothing to add is not
 * written and words [W, bits_ld) are never touched.  max_ts >= 0 and max_initial count timestamp units.  The result is
 * the same bits in every run.  Limits as tmi_decode_constraints (M <= 65535, V <= 65536, t <= 65536), 0 <= tb <= V,
 * no_timestamps_id and eos_id < V (negative: none); anything else is TMI_ERR_INVALID and launches nothing.
 *
 * tmi_lm_head_timestamp_gate: g for M rows in one launch that streams the LM head once: x .. V and seen, banned, bits_ld,
 * penalty as for tmi_lm_head_argmax_c (seen may be NULL; banned is required and written), z' by the same device code in
 * the same accumulation order as the _c kernels, so a column's z' here is bit for bit the z' the step's head then sees.
 * Per workgroup (max_below) and (max_ts, sum exp) partials meet in `workspace` and are folded in a fixed column order,
 * as tmi_lm_head_topk folds its lse: bit-reproducible.  fired[r] (int32 [M]) = 1 where the rule fired, else 0; where it
 * fired the below columns are OR-ed into banned[r], nothing else of banned changes, seen is not written.
 * Ordering: every workgroup of the launch reads the row's banned words, so they are rewritten inside the SAME launch by
 * the last workgroup of the row's 16-row tile to arrive, after every partial of that tile is in (the completion counter
 * that tmi_lm_head_topk uses to clean its workspace); there is no second launch.
 * `workspace`: >= tmi_lm_head_timestamp_gate_workspace_bytes(M, V) = 16 * M * (1 + ceil(V / 128)) bytes (-1 for sizes the
 * kernel refuses), 16-byte aligned, ZERO before the first call and left zero by every call; one buffer per stream.
 * V <= 65536, 0 <= tb <= V, the LDS bound of tmi_lm_head_argmax; anything else is TMI_ERR_INVALID and launches nothing.
 */
int tmi_timestamp_rules(const int32_t* prefix, int64_t ld, int64_t M, int64_t t, int64_t P, int64_t V, int64_t tb,
                        int32_t no_timestamps_id, int32_t eos_id, int64_t max_initial, int64_t max_ts, uint32_t* banned,
                        int64_t bits_ld, void* stream);
int64_t tmi_lm_head_timestamp_gate_workspace_bytes(int64_t M, int64_t V);
int tmi_lm_head_timestamp_gate(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, float eps,
                               const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                               const uint32_t* seen, uint32_t* banned, int64_t bits_ld, float penalty, int64_t tb,
                               int32_t* fired, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * One step of beam search's bookkeeping (the rule of whisper.py generate / INTEGRATION.md), one workgroup per batch item
 * b of B; row r = b * K + k is beam k (1 <= K <= 8).  Step t (finalize = 0; 2K <= N <= 16):
 *   candidates (k, cand_ids[r * N + j], sums[r] + cand_lp[r * N + j]) (fp32 add), ranked by score desc then (k, id) asc;
 *   the first 2K are walked: EOS (eos_id >= 0) at rank < K offers cur[r, :t] + [EOS] (length t, score / len_pow) to the
 *   pool, at rank >= K is skipped; any other becomes the next live beam n: nxt[b*K + n, :t+1] = cur[parent, :t] + [id],
 *   sums[b*K + n] = score.  The pool (pool_ids [B, K, ld], pool_scores / pool_len [B, K], pool_cnt [B]) stays sorted by
 *   score desc then insertion; it admits while not full, then replaces its last entry only on a strictly greater score.
 *   done[b] = 1 and done_count[0] += 1 once the pool is full and early_stopping or pool_scores[b, K-1] >= (best new live
 *   sum) / len_pow.  An item that is done is frozen: only nxt[r, :t] = cur[r, :t] is written.
 * finalize = 1: every item not done offers its K live beams cur[r, :t+1] (length t, score sums[r] / len_pow) in order
 *   k = 0..K-1; cand_ids, cand_lp and nxt are not read.
 * len_pow = t ** length_penalty (fp32, finite, > 0) is the caller's, so that a host restatement rounds identically; the
 * divisions are correctly rounded.  1 <= t < ld.
 */
int tmi_beam_step(const int32_t* cand_ids, const float* cand_lp, int64_t N, int64_t B, int64_t K, float* sums,
                  const int32_t* cur, int32_t* nxt, int64_t ld, int64_t t, int32_t eos_id, float len_pow,
                  int32_t early_stopping, int32_t* pool_ids, float* pool_scores, int32_t* pool_len, int32_t* pool_cnt,
                  int32_t* done, int32_t* done_count, int32_t finalize, void* stream);

/* ------------------------------------------------------------------------------------
 * Teacher-forced scoring without a whole-vocabulary buffer (whisper.py evaluate / score: the loss of W:585-600 and the
 * SparseCategoricalAccuracy of W:904-907, forward only).  The caller evaluates the LM head in column chunks with tmi_gemm -
 * chunk c holds the columns [col0, col0 + ncols) of the logits z[M, V..] as chunk[r * ld + j] = z[r, col0 + j] (dtype: F32
 * or BF16) - and calls this once per chunk, in ascending col0, on one stream.  Running state per row r, in `state`:
 *   (m_r, s_r)  max and sum exp(z - m_r) over the real columns n < V seen so far (fp32 online softmax).  Inside a chunk
 *               lane l of the row's wave folds its 16-byte vectors (8 bf16 / 4 fp32 columns at j = (l + 64 i) * 8 or * 4)
 *               in ascending i, the 64 lane partials meet in a butterfly (lane distance 32, 16, .., 1) in which the lower
 *               lane's pair is folded first, and the chunk's pair is folded behind the running one: for a fixed sequence of
 *               (col0, ncols) every output is bit-reproducible;
 *   best_r      argmax over n < V: the largest stored logit, the smallest column among equals (-0 == +0), as a 64-bit key
 *               (order-preserving float bits << 32 | ~n, tmi_lm_head_argmax's); a chunk's best replaces the running best
 *               only when strictly greater, so the earlier chunk wins a tie;
 *   zt_r        the target logit, taken in the chunk with col0 <= targets[r] < col0 + ncols: read from the chunk (zts_r); for
 *               BF16 chunks with x and w given also recomputed as x[r * x_ld + k] . w[k * w_sk + targets[r] * w_sn], k < d,
 *               in fp32 from the bf16 operands the GEMM read (the note on tmi_linear_xent says why).  F32 chunks ignore x, w.
 * first = 1 (exactly when col0 == 0) initialises the state from this chunk: the buffer needs no zeroing and may hold
 * anything.  last = 1 (exactly when col0 + ncols >= V) also writes, for every row,
 *   lse[r] = m_r + log(s_r);   argmax[r] = best column (int32);
 *   logprob[r] = 0 for targets[r] == -1, else zts_r - lse[r] without a recomputed target logit, else tmi_linear_xent's form
 *                -log1p(rest * exp(m_r - zt_r)), rest = max(s_r - exp(zts_r - m_r), 0): the log-softmax with the target's own
 *                term of the sum taken at the recomputed zt_r too, so that both terms see the same target logit (never
 *                positive; with the stored lse a dominating target would keep half a bf16 ulp of its logit as error).
 * targets[r] = -1: the row is not scored (lse and argmax are still written).  The pad columns n >= V of a chunk are never
 * read into any of the three (they may hold anything, NaN included).  Out-of-range targets: the values live in device
 * memory, so the call does not see them; a target outside [-1, V) is never dereferenced and gives logprob[r] = NaN (the
 * Python wrapper ops.logprob_fold checks the range on the host before the first chunk).
 * Everything else is validated before anything is launched, and a rejected call writes nothing: chunk 16-byte aligned, ld
 * a multiple of 8 (BF16) / 4 (F32) and >= ncols >= 1, 1 <= V, 0 <= col0 < V, M >= 1, and M, V, ld <= 2^30 (the kernel
 * indexes rows and columns with 32-bit integers); targets 4-byte aligned; x and w both given or both NULL (2-byte aligned,
 * 1 <= d <= 2^20, x_ld >= d, nonzero w strides); state 8-byte aligned with state_bytes >= tmi_logprob_state_bytes(M) =
 * 32 * M; first / last in {0, 1} and consistent with col0 / ncols / V; lse / logprob / argmax non-NULL and 4-byte aligned
 * when last = 1 (ignored otherwise).
 * No atomics, no workspace besides the caller-owned state.  tmi_logprob_chunk_cols(): the chunk width the library's callers
 * use (a multiple of the GEMM's widest N tile; measured, DESIGN.md "Evaluation").
 */
int64_t tmi_logprob_state_bytes(int64_t M);
int64_t tmi_logprob_chunk_cols(void);
int tmi_logprob_fold(const void* chunk, int64_t ld, int32_t dtype, int64_t M, int64_t V, int64_t col0, int64_t ncols,
                     const int32_t* targets, const void* x, int64_t x_ld, const void* w, int64_t w_sk, int64_t w_sn,
                     int64_t d, void* state, int64_t state_bytes, int32_t first, int32_t last, float* lse, float* logprob,
                     int32_t* argmax, void* stream);

/* ------------------------------------------------------------------------------------
 * Multi-tensor Adam over a flat fp32 arena (tf.keras.optimizers.Adam, W:901; V:1271-1275).
 *   g' = g * gscale                      (gscale: 1 for Whisper's SUM, 1/N for V:1231)
 *   m <- b1 m + (1-b1) g' ; v <- b2 v + (1-b2) g'^2
 *   eps_mode 0 (TF/Keras-V2): p <- p - lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
 *   eps_mode 1 (torch):       p <- p - lr * (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps)
 *   weight_decay (decoupled, AdamW) defaults to 0 in the reference.
 * bf16_mirror (optional, may be NULL): bf16 copy of the updated parameters, same flat
 * indexing — the k-contiguous / natural-layout weight operand of the bf16 GEMMs.
 * zero_grad != 0: g is overwritten with zeros once consumed (the next backward accumulates into it; saves the
 * separate fill pass).  max_blocks > 0 caps the grid: a slice of the arena updated beside other kernels (the
 * optimizer running bucket by bucket under backward) must leave them the CUs.
 * Algorithmic traffic: 28 B/param (read p,g,m,v; write p,m,v) + 2 B/param for the mirror (+ 4 with zero_grad).
 */
int tmi_adam_step(float* p, float* g, float* m, float* v, int64_t n, float lr,
                  float beta1, float beta2, float eps, int32_t step, int32_t eps_mode,
                  float weight_decay, float gscale, void* bf16_mirror, int32_t zero_grad,
                  int32_t max_blocks, void* stream);
/* The same update over an embedding table [nrows][row_len] (tf.keras.layers.Embedding, W:382), skipping idle rows:
 * a row whose gradient is all zero and that has never been updated (active[r] == 0: m = v = 0) has an exactly-zero
 * Adam update, so only its gradient is read.  active: one byte per row, zero-initialised by the caller and kept
 * across steps (set by the kernel the first time a row sees a gradient).  weight_decay must be 0. */
int tmi_adam_step_rows(float* p, float* g, float* m, float* v, int64_t nrows, int64_t row_len,
                       unsigned char* active, float lr, float beta1, float beta2, float eps,
                       int32_t step, int32_t eps_mode, float weight_decay, float gscale,
                       void* bf16_mirror, int32_t zero_grad, void* stream);
/* tmi_adam_step over the reference's variables (chunks: int64 device array [nchunks][3] = (first element, end element,
 * variable index) tiling the arena in pieces that never cross a variable; sumsq indexed by variable) with the gradient clipping of V:1243 (tf.clip_by_global_norm, before the update) and V:1274 (Keras
 * clipnorm = tf.clip_by_norm per variable) applied as a per-variable factor of g, computed from ONE
 * tmi_segment_sumsq pass over the raw gradients (sumsq[nseg]):
 *   c_g = clip_global / max(||g||, clip_global),  c_s = clip_each / max(c_g * ||g_s||, clip_each),  g' = g * gscale * c_g * c_s
 * (clip_global == 0 / clip_each == 0 switch a stage off).  No clipped copy of the gradients is written. */
int tmi_adam_step_segments(float* p, float* g, float* m, float* v, const int64_t* chunks,
                           int64_t nchunks, const float* sumsq, int64_t nseg, float clip_global, float clip_each, float lr,
                           float beta1, float beta2, float eps, int32_t step, int32_t eps_mode,
                           float weight_decay, float gscale, void* bf16_mirror, int32_t zero_grad,
                           int32_t max_blocks, void* stream);
/* (max_blocks > 0 caps the grid, as in tmi_adam_step: for a slice of the table that runs beside other work.  The global
 * norm always comes from the whole sumsq[nseg], so a sub-table of chunks is the same update restricted to its rows.) */
/* The step-dependent scalars of tmi_adam_step, computed on the host exactly as it does:
 * out3 = {step_size, vcorr_inv_sqrt, 1 - lr*weight_decay}. */
int tmi_adam_scalars(float lr, float beta1, float beta2, int32_t step, int32_t eps_mode,
                     float weight_decay, float* out3);
/* tmi_adam_step with those three scalars read from DEVICE memory (dev_scalars[3]): nothing in the
 * launch changes from step to step, so it can be part of a captured HIP graph. */
int tmi_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float beta1,
                      float beta2, float eps, const float* dev_scalars, int32_t eps_mode,
                      float gscale, void* bf16_mirror, void* stream);


/* Gradient exchange staging (C1, W:834 / V:1246: the implicit cross-replica SUM of every gradient; the
 * exchange itself is RCCL through torch.distributed, these are the device-side passes around it).
 * tmi_grad_pack:   dst[i] = bf16(src[i] * scale) - an fp32 arena slice onto a bf16 wire buffer.
 * tmi_grad_unpack: dst[i] = scale * sum_{p < nparts} src[p*part_stride + i], src bf16 or fp32, fp32 sum:
 *   the widening of a reduced bf16 bucket (nparts = 1) and the local reduction of the nparts pieces a mesh
 *   reduce-scatter (all-to-all over the xGMI links) delivers. */
int tmi_grad_pack(const float* src, void* dst, int64_t n, float scale, void* stream);
int tmi_grad_unpack(const void* src, int32_t src_dtype, int64_t nparts, int64_t part_stride, float* dst,
                    int64_t n, float scale, void* stream);

/* bf16 shadows of fp32 master weights: dst[r*ldd + c] = bf16(src[r*lds + c]) and the
 * transposed form dst[c*ldd + r] = bf16(src[r*lds + c]); pad columns [cols, ldd) of the
 * plain form are written as zero. */
int tmi_cast_bf16(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t rows,
                  int64_t cols, void* stream);
int tmi_transpose_cast_bf16(const float* src, int64_t lds, void* dst, int64_t ldd,
                            int64_t rows, int64_t cols, void* stream);

/* features [B, C, T] fp32 (W:792 layout) -> channels-last, time-padded
 * out[b, pad_left + t, c] of shape [B, T + pad_left + pad_right, C] (pad rows zeroed):
 * the tf.transpose of W:329 fused with the "same" padding of W:311. */
int tmi_feat_to_channels_last(const float* feats, void* out, int64_t B, int64_t C, int64_t T,
                              int64_t pad_left, int64_t pad_right, int32_t dtype, void* stream);

/* sum of squares of n fp32 values into out[0] (+= if accumulate): tf.clip_by_global_norm
 * (V:1243) first stage. */
int tmi_sumsq(const float* x, float* out, int64_t n, int32_t accumulate, void* stream);

/* ====================================================================================
 * Wav2Vec2 pre-training path (speech_jobs/wav2vec2_dist.py, "V:")
 * ==================================================================================== */

/* GroupNormalization (V:140-196; contiguous channel groups, statistics over (time, C/G) per
 * (batch, group), biased variance, per-channel affine) fused with the exact-erf GELU that
 * follows it in every conv layer of the feature encoder (V:283-288):
 *   y[b,t,c] = gelu(gamma[c] * (x - mean[b,g]) * rstd[b,g] + beta[c])
 * x is [B][T][C] with batch stride x_sb, y likewise with y_sb (so y may be the padded input
 * buffer of the next Conv1D).  stats: fp32 [B,G,2] = (mean, rstd), saved for backward.
 * part: fp32 workspace [B * tmi_groupnorm_chunks(T) * G * 2].
 * Backward: dx = d/dx of the above given dy (GELU' recomputed from x and stats);
 * dgamma/dbeta are ACCUMULATED (atomics; caller zeroes); sums: fp32 workspace [B,G,2]. */
int64_t tmi_groupnorm_chunks(int64_t T);
int tmi_groupnorm_gelu_fwd(const void* x, int64_t x_sb, const float* gamma, const float* beta,
                           void* y, int64_t y_sb, float* stats, float* part, int64_t B, int64_t T,
                           int64_t C, int64_t G, float eps, int32_t dtype, void* stream);
int tmi_groupnorm_gelu_bwd(const void* x, int64_t x_sb, const void* dy, int64_t dy_sb,
                           const float* gamma, const float* beta, const float* stats, void* dx,
                           int64_t dx_sb, float* dgamma, float* dbeta, float* part, float* sums,
                           int64_t B, int64_t T, int64_t C, int64_t G, int32_t dtype, void* stream);

/* Layout packs that turn the grouped positional Conv1D (V:271-277: k = 128, groups = 16,
 * "same") into ONE batched tmi_gemm over overlapping rows:
 *   tmi_group_pack:   x [B*T][C] -> xg [G][B*Tp][C/G], batch b's rows at [b*Tp + pad_left, +T),
 *                     every other row zero (the "same" padding, and zero rows for the gradient);
 *   tmi_group_unpack: out[b*T+t][g*Cg+j] = yg[g][b*Tp + t + row_off][j] (+ bias[c]) (+ resid);
 *   tmi_posconv_pack_weights: Keras kernel w [k][C/G][C] fp32 -> forward operand
 *                     wf[g][(kk,i)][o] = w[kk][i][g*Cg+o] and backward operand
 *                     wb[g][(kk',o)][i] = w[k-1-kk'][i][g*Cg+o] (both [G][k*Cg][Cg], dtype). */
int tmi_group_pack(const void* x, void* xg, int64_t B, int64_t T, int64_t C, int64_t G, int64_t Tp,
                   int64_t pad_left, int32_t dtype, void* stream);
int tmi_group_unpack(const void* yg, const float* bias, const void* resid, void* out, int64_t B,
                     int64_t T, int64_t C, int64_t G, int64_t Tp, int64_t row_off, int32_t dtype,
                     void* stream);
int tmi_posconv_pack_weights(const float* w, void* wf, void* wb, int64_t k, int64_t Cg, int64_t G,
                             int32_t dtype, void* stream);

/* Hard vector quantiser (V:581-667): per row and group, squared L2 to every code computed as
 * sum((h-c)^2) in fp32, tf.argmin (first index on ties), q = the chosen code;
 * perplexity[0] = mean_g exp(-sum_c p log(p+1e-10)), p = clip(mean one-hot, 1e-10, 1).
 * h, q: [rows][G*gd] (dtype); codebook fp32 [G][Nc][gd]; idx int32 [rows][G].
 * tmi_vq_bwd: dcodebook[g][idx][:] += dq (the only gradient path of the quantiser, V:638). */
int tmi_vq_nearest(const void* h, const float* codebook, int32_t* idx, void* q, float* perplexity,
                   int64_t rows, int64_t G, int64_t Nc, int64_t gd, int32_t dtype, void* stream);
/* The same quantiser with the code choice given (idx is an INPUT, clamped to [0, Nc)): q = the chosen codes, the same
 * perplexity.  For replaying a recorded code sequence (teacher-forced parity runs of the bf16 path). */
int tmi_vq_assign(const float* codebook, const int32_t* idx, void* q, float* perplexity, int64_t rows,
                  int64_t G, int64_t Nc, int64_t gd, int32_t dtype, void* stream);
int tmi_vq_bwd(const int32_t* idx, const void* dq, float* dcodebook, int64_t rows, int64_t G,
               int64_t Nc, int64_t gd, int32_t dtype, void* stream);

/* First feature-encoder layer as a filter bank (V:283-288, i = 0: Conv1D(C, kernel 10, stride 5, "same", no bias) on
 * the single-channel audio, then GroupNorm (V:140-196) and exact GELU), never materialising the conv output: both
 * passes of the forward and both passes of the backward recompute it from the raw audio with the taps in registers.
 *   audio fp32 [B][Tin] (batch stride a_sb); w fp32 [k][C] (the Keras kernel [k, 1, C]); T = ceil(Tin / stride) output
 *   steps, pad_left = the "same" padding on the left; y / dy [B][T][C] of `dtype` with their own batch strides.
 *   fwd: stats[B][G][2] = (mean, rstd) of u = conv(audio), y = gelu(gamma * xhat + beta).
 *   bwd: dW[k][C] += d/dw, dgamma[C] += .., dbeta[C] += ..  (no input gradient: the input is data).
 *   part: fp32 scratch of tmi_fir_chunks(T)*B*G*2 floats; sums: [B][G][2]; wpart: tmi_fir_gn_workspace_floats(). */
int64_t tmi_fir_chunks(int64_t T);
int64_t tmi_fir_gn_workspace_floats(int64_t B, int64_t T, int64_t C);
int tmi_fir_groupnorm_gelu_fwd(const float* audio, int64_t a_sb, int64_t Tin, int64_t pad_left, const float* w,
                               int64_t k, int64_t stride, const float* gamma, const float* beta, void* y,
                               int64_t y_sb, float* stats, float* part, int64_t B, int64_t T, int64_t C,
                               int64_t G, float eps, int32_t dtype, void* stream);
int tmi_fir_groupnorm_gelu_bwd(const float* audio, int64_t a_sb, int64_t Tin, int64_t pad_left, const float* w,
                               int64_t k, int64_t stride, const void* dy, int64_t dy_sb, const float* gamma,
                               const float* beta, const float* stats, float* dW, float* dgamma, float* dbeta,
                               float* part, float* sums, float* wpart, int64_t B, int64_t T, int64_t C,
                               int64_t G, int32_t dtype, void* stream);

/* Contrastive loss (V:866-899; whisper_single.py:745-787) on S [B][T][T] fp32 = all-pairs <h_t, q_t'>
 * (a tmi_gemm): row (b,t) has logits [S[t][t], S[t][idx[0..Nn)]] / temperature and label 0, where
 * idx = neg + b*neg_sb + t*neg_st (element strides): V:908-937 draws one row of indices per batch row
 * (neg [B][Nn]: neg_sb = Nn, neg_st = 0); whisper_single.py:789-839 one row per time step, shared by
 * the batch (neg [T][Nn]: neg_sb = 0, neg_st = Nn).  Indices may repeat and may equal t.
 * row_loss[b*T+t] = logsumexp - logit_0; S is REPLACED by d(sum row_loss)/dS * grad_scale. */
int tmi_contrastive_fwd_bwd(float* S, const int32_t* neg, int64_t neg_sb, int64_t neg_st,
                            float* row_loss, int64_t B, int64_t T, int64_t Nn, float temperature,
                            float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------
 * Wav2Vec2 evaluation (wav2vec2.py evaluate): the contrastive loss of V:866-899 and its argmax accuracy in GATHERED form,
 * forward only - O(T * Nn * pd) dot products, no [T, T] product, no gradient - with a rule for padded frames.
 *   h, q   [B][T][pd] of `dtype` (TMI_F32 / TMI_BF16): element (b, t, k) at (b * T + t) * ld + k, ld >= pd, so the call takes
 *          column slices of wider buffers;
 *   neg    int32, row (b, t) reads neg[b * neg_sb + t * neg_st + n], n < Nn, exactly as tmi_contrastive_fwd_bwd does
 *          ([B][Nn]: neg_sb = Nn, neg_st = 0; [T][Nn]: neg_sb = 0, neg_st = Nn).  Indices may repeat and may equal t;
 *   mask   fp32 [B][T] or NULL (all ones): frame (b, t) is VALID iff mask[b * T + t] > 0.
 * Row (b, t) of a valid frame: logits z_0 = <h_t, q_t> / temperature, then z_n = <h_t, q_j> / temperature for every
 * j = neg[..][n - 1] whose frame (b, j) is valid; a negative that names a masked frame is dropped from the row's softmax.
 *   row_loss[b * T + t]    = logsumexp(z) - z_0, computed as (max - z_0) + log(sum exp(z - max)): never rounded at the size
 *                            of the logits, never negative;
 *   row_correct[b * T + t] = 1 iff z_0 >= every kept z_n (tf.argmax takes the first index on a tie; index 0 is the positive);
 *   a row that keeps no negative has loss 0 and correct 1.  Row (b, t) of a masked frame: loss 0, correct 0.
 * Arithmetic (one wave per row; lane l owns the items l, l + 64, .. of [positive, negatives]): every logit, the positive's
 * included, is ONE code path - an fp32 fma chain over k = 0 .. pd-1 in ascending k from the stored operands, times
 * fl(1 / temperature) - so a negative equal to t ties the positive bit for bit and the row counts as correct.  A lane folds
 * its items in ascending order into an online (max, sum exp) pair; the row maximum is the exact maximum of the lane maxima,
 * each lane rescales its sum once by expf(lane max - row max), and the 64 sums are added in a butterfly (lane distance 32,
 * 16, .., 1).  No float atomics, no workspace: two runs are bit-identical.
 * Index VALUES live in device memory and are not seen by the call: an index outside [0, T) is never dereferenced and is
 * dropped like a masked frame (the Python wrapper ops.contrastive_score checks 0 <= idx < T on the host first).  Everything
 * else is validated before anything is launched, and a rejected call writes nothing: non-NULL h, q, neg, row_loss,
 * row_correct; h and q 16-byte aligned, the rest 4-byte; pd and ld multiples of 8 (BF16) / 4 (F32), ld >= pd; B, T, Nn >= 1;
 * B, T, Nn, pd, ld and B * T <= 2^30; neg_sb, neg_st >= 0; temperature > 0. */
int tmi_contrastive_score(const void* h, const void* q, int64_t ld, int32_t dtype, const int32_t* neg, int64_t neg_sb,
                          int64_t neg_st, const float* mask, float* row_loss, int32_t* row_correct, int64_t B, int64_t T,
                          int64_t pd, int64_t Nn, float temperature, void* stream);

/* Code usage of an evaluation set: counts[g * Nc + c] += 1 for every VALID row r (mask[r] > 0; mask fp32 [rows] or NULL:
 * all rows) and group g with c = clamp(idx[r * G + g], 0, Nc - 1) - the clamp of tmi_vq_assign, so the code counted is the
 * code assigned.  idx int32 [rows][G], counts int64 [G][Nc] (8-byte aligned).  The call ACCUMULATES: the caller zeroes
 * counts once per evaluation and reads it once at the end.  Integer adds only (an LDS histogram per workgroup, then 64-bit
 * global atomic adds): the result is exact and independent of order.  1 <= rows <= 2^30, G * Nc <= 8192 (tmi_vq_nearest's
 * limit); a rejected call writes nothing. */
int tmi_vq_count(const int32_t* idx, const float* mask, int64_t* counts, int64_t rows, int64_t G, int64_t Nc, void* stream);

/* Gradient clipping.  seg_off: int64 device array [nseg+1] of element offsets into g.
 * tmi_segment_sumsq: out[s] = sum g[seg_off[s]:seg_off[s+1]]^2.
 * tmi_segment_clip:  g[seg s] *= clip / max(sqrt(sumsq[s]), clip).
 * One segment covering the arena = tf.clip_by_global_norm (V:1243); one segment per variable
 * = Keras clipnorm (V:1274). */
int tmi_segment_sumsq(const float* g, const int64_t* seg_off, float* out, int64_t nseg, void* stream);
/* The same sums over the chunk table of tmi_adam_step_segments ([nchunks][3] = lo, hi, segment index): equal pieces of work
 * instead of one workgroup row per segment.  out[nseg] is zeroed first. */
int tmi_segment_sumsq_chunks(const float* g, const int64_t* chunks, int64_t nchunks, float* out, int64_t nseg, void* stream);
int tmi_segment_clip(float* g, const int64_t* seg_off, const float* sumsq, int64_t nseg, float clip,
                     void* stream);

/* out[0] = nan_to_zero(a[0] + w * b[0]) * scale  (V:1220-1231: contrastive + 0.1 * (-perplexity),
 * NaN guard, / num_replicas) without a host round trip. */
int tmi_loss_combine(const float* a, const float* b, float w, float scale, float* out, void* stream);

/* Masked mean over time, the reduction of the reference's classification head (V:1031-1042):
 *   out[b, c] = sum_t x[b, t, c] * mask[b, t] / sum_t mask[b, t]
 * x [B, T, C] contiguous (x_dtype TMI_F32 or TMI_BF16, 16-byte aligned, C a multiple of 4 resp. 8), mask [B, T] fp32 or
 * NULL for the plain mean over T (V:1042), out [B, C] fp32.  Accumulated in fp32 in a fixed order without atomics: two
 * runs are bit-identical.  Deviation from the reference: a batch row whose mask sums to zero yields zeros, where the
 * reference's 0 / 0 yields NaN. */
int tmi_masked_mean_pool(const void* x, int32_t x_dtype, const float* mask, float* out, int64_t B, int64_t T, int64_t C,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * The sequence-classification head (Wav2Vec2ForSequenceClassification, V:1045-1056) on pooled features, fp32 throughout.
 * N rows; row r of the call reads pooled[s * ld_x .. + H) with s = row_index ? row_index[r] : r (row_index int32 [N] or
 * NULL; n_src = the rows `pooled` holds: an index outside [0, n_src) reads as a row of zeros).  Wp [H, P], bp [P],
 * Wc [P, C], bc [C] contiguous.
 *
 * tmi_cls_head_fwd, per row r:
 *   pre[c]    = (fmaf(x[h], Wp[h][c], .) over h = 0 .. H-1 in that order, from 0) + bp[c]
 *   z[c]      = tanhf(pre[c])
 *   y[c]      = keep(seed, r, c) ? z[c] * 65536/(65536-thr) : 0    tmi_dropout's generator exactly: stream 0, row = r (the
 *               position in THIS call, not the source row), column = c, 16-bit draws, thr = round(p * 65536); p == 0: y = z
 *               and nothing is hashed (the seed is ignored)
 *   logits[k] = (fmaf(y[c], Wc[c][k], .) over c = 0 .. P-1 in that order, from 0) + bc[k]
 *   m = max_k logits[k];  s = sum_k expf(logits[k] - m): lane l of a wave adds its classes l, l + 64, .. in ascending
 *               order from 0, then the xor butterfly 32, 16, .., 1 folds the 64 lanes;  lse = m + logf(s)
 *   log_probs[k] = logits[k] - lse
 *   pred      = the lowest k with logits[k] == m (numeric comparison: -0 ties with +0)
 *   labelled rows (labels non-NULL and 0 <= labels[r] < C):
 *     nll        = -(logits[label] - lse)       (= -log_probs[label], bit for bit)
 *     label_rank = #{k : logits[k] > logits[label]} + #{k < label : logits[k] == logits[label]}
 *                  so label_rank < n means "the label is in the top n", and label_rank == 0 exactly when pred == label
 *     confusion[label * ld_conf + pred] += 1    (int64, global integer atomics: order cannot change the result; the
 *                  caller zeroes the table, or passes the previous one in to accumulate)
 *   unlabelled rows: nll = 0, label_rank = -1, no table update.
 * logits [N, ld_logits] and pred [N] are always written; z [N, ld_z] (the tanh output BEFORE dropout: what the backward
 * takes), log_probs [N, ld_lp], nll [N], label_rank [N] and confusion may be NULL.  Nothing else is written; no
 * floating-point atomic: the same call gives the same bits.
 *
 * tmi_cls_head_bwd: the gradients of loss = (sum over labelled rows of nll) / n_valid, from the z and log_probs the
 * forward saved and the same (p, seed); no mask is stored, y is recomputed.
 *   n_valid   = the number of labelled rows, counted on the device (integer)
 *   loss[0]   = (thread t of 256 adds -log_probs[r][label] of rows t, t + 256, .. ascending; wave butterflies; the four wave
 *               sums in order) / n_valid; 0 when n_valid == 0
 *   dlogits[r][k] = (expf(log_probs[r][k]) - (k == label)) * (1 / n_valid) on labelled rows, 0 elsewhere
 *   gbc[k]    = sum_r dlogits[r][k]               gWc[c][k] = fmaf(y[r][c], dlogits[r][k], .)  both over r ascending (*)
 *   dy[r][c]  = fmaf(dlogits[r][k], Wc[c][k], .) over k ascending
 *   dpre[r][c] = (keep(seed, r, c) ? dy * scale : 0) * fmaf(-z, z, 1)     (a saturated tanh, z = +-1, gives exactly 0)
 *   gbp[c]    = sum_r dpre[r][c]                  gWp[h][c] = fmaf(x[r][h], dpre[r][c], .)     both over r ascending (*)
 *   (*) N <= 256: one chain from 0 over r = 0 .. N-1.  N > 256: one such chain per chunk of 256 consecutive rows, then the
 *       chunks' sums added in ascending order.  The order depends on N alone.
 * Gradients (gWp [H, P], gbp [P], gWc [P, C], gbc [C], contiguous) are written, not accumulated; with n_valid == 0 all are
 * zero.  workspace: tmi_cls_head_workspace_bytes(N, H, P, C) bytes, 16-byte aligned, any contents; afterwards a 256-byte
 * header (int32 n_valid first), dpre [N, P] behind it and, for N > 256, the chunks' partial sums behind that.
 *
 * Limits, both calls: 1 <= N <= 65535; 4 <= H <= 4096, a multiple of 4; 2 <= P <= 1024, even; 1 <= C <= 1024; 0 <= p < 1;
 * row strides >= the row and <= 2^30; without a row_index n_src >= N.  Anything else: TMI_ERR_INVALID, nothing is launched
 * and nothing written.  tmi_cls_head_workspace_bytes returns -1 outside the limits. */
int64_t tmi_cls_head_workspace_bytes(int64_t N, int64_t H, int64_t P, int64_t C);
int tmi_cls_head_fwd(const float* pooled, int64_t ld_x, int64_t n_src, const int32_t* row_index, const float* Wp,
                     const float* bp, const float* Wc, const float* bc, const int32_t* labels, float p, uint64_t seed,
                     float* logits, int64_t ld_logits, int32_t* pred, float* z, int64_t ld_z, float* log_probs, int64_t ld_lp,
                     float* nll, int32_t* label_rank, int64_t* confusion, int64_t ld_conf, int64_t N, int64_t H, int64_t P,
                     int64_t C, void* stream);
int tmi_cls_head_bwd(const float* pooled, int64_t ld_x, int64_t n_src, const int32_t* row_index, const float* Wc,
                     const int32_t* labels, float p, uint64_t seed, const float* z, int64_t ld_z, const float* log_probs,
                     int64_t ld_lp, float* gWp, float* gbp, float* gWc, float* gbc, float* loss, void* workspace,
                     int64_t workspace_bytes, int64_t N, int64_t H, int64_t P, int64_t C, void* stream);

/* ------------------------------------------------------------------------------------
 * The CTC head on cached encoder features (Wav2Vec2ForCTC, V:972-975: Dropout, then Dense), for training the head with
 * the encoder frozen (csrc/ctc_head.hip).  fp32 throughout, from fp32 W [H, V] and b [V] (contiguous).  `hidden` holds the
 * encoder's output in x_dtype (TMI_BF16 or TMI_F32): element (s, t, h) at hidden[s*x_sn + t*x_st + h].  N items per call,
 * T_max frames each; item n reads source item s = row_index ? row_index[n] : n (row_index int32 [N] or NULL; n_src = the
 * items `hidden` holds: an index outside [0, n_src) reads as zeros).  frame_lens, label_lens, nll, infeasible are BY
 * POSITION n in the call, as tmi_ctc_posteriors takes and writes them; only `hidden` is gathered.  T = min(frame_lens[n],
 * T_max); row r = n*T_max + t is LIVE when t < T.  Frames t >= T, and every frame of an item with frame_lens[n] < 1, are
 * neither read nor written by these calls.
 *
 * tmi_ctc_head_fwd, per live row:
 *   xd[h]     = keep(seed, r, h) ? x[h] * 65536/(65536-thr) : 0    tmi_dropout's generator exactly: stream 0, row = r =
 *               n*T_max + t (the position in THIS call, not the source row), column = h, 16-bit draws, thr = round(p * 65536),
 *               the scale formed in fp32 as tmi_cls_head_fwd forms it; p == 0: xd = x, nothing is hashed, the seed is ignored
 *   logits[v] = (fmaf(xd[h], W[h][v], .) over h = 0 .. H-1 in that order, from 0) + b[v]
 *   m = max_v logits[v];  s = sum_v expf(logits[v] - m): column v on lane v of a wave, the lanes past V hold 0, folded by the
 *               xor butterfly 32, 16, .., 1;  lse = m + logf(s);  logp[v] = logits[v] - lse   (tmi_ctc_logsoftmax's form)
 *   argmax    = the smallest column among equal maxima of the logits (tmi_ctc_logsoftmax's rule)
 * logp (element (n, t, v) at logp[n*lp_sn + t*lp_st + v]) is always written; logits (the same layout under lg_sn / lg_st)
 * and argmax (int32 [N][T_max], dense) may be NULL.  Columns past V are not written.
 *
 * tmi_ctc_head_bwd: the gradients of loss = sum_n w_n nll[n] with respect to W and b, from `grad` as tmi_ctc_posteriors
 * wrote it (d nll[n] / d logits, element (n, t, v) at grad[n*gr_sn + t*gr_st + v]), its nll [N] and infeasible [N], and the
 * same hidden, row_index, frame_lens and (p, seed) as the forward; no mask is stored, xd is recomputed.
 *   w_n       = 0 when infeasible[n] != 0; else 1 (reduction 0, "sum") or 1 / ((float) max(min(label_lens[n], L_max), 1) *
 *               (float) N) (reduction 1, "mean": torch's ctc_loss(reduction="mean", zero_infinity=True))
 *   gs[r][v]  = grad[r][v] * w_n on a live row; a row that is not live counts as zeros and is not read
 *   gW[h][v]  = fmaf(xd[r][h], gs[r][v], .)       gb[v] = sum of gs[r][v]       both over the rows r ascending (*)
 *   (*) the rows 0 .. N*T_max - 1 are cut into chunks of rc = 256 * ceil(N*T_max / 16384) consecutive rows (256 rows up to
 *       N*T_max = 16384; at most 64 chunks).  Per chunk one chain from 0 over its rows in ascending order; then the chunks'
 *       sums are added in ascending chunk order, starting from chunk 0's.  The order depends on N*T_max alone.
 *   loss[0]   = sum over the feasible items of w_n * nll[n] (one product, then added): thread t of 256 adds its items t,
 *               t + 256, .. in ascending order from 0, the 64 lanes of a wave meet in the xor butterfly 32, 16, .., 1, the four
 *               wave sums are added ((w0 + w1) + w2) + w3.  An infeasible item's nll is not read into the sum.
 *   n_infeasible[0] = the number of items with infeasible[n] != 0 (int32)
 * gW [H, V], gb [V] (contiguous), loss and n_infeasible are written, not accumulated; with no live row gW and gb are zero.
 * No floating-point atomic anywhere: the same call gives the same bits.  workspace: tmi_ctc_head_workspace_bytes(N, T_max,
 * H, V) bytes (the chunks' partial sums, chunks * (H*V + V) floats), 16-byte aligned, any contents.
 *
 * Limits, both calls: 1 <= N <= 65535; 1 <= T_max <= 4096; N*T_max <= 2^22; 8 <= H <= 4096, a multiple of 8; 2 <= V <= 64;
 * 0 <= p < 1; frame strides >= the row (x_st >= H; lp_st, lg_st, gr_st >= V), item strides >= T_max * the frame stride, all
 * <= 2^30; 1 <= n_src <= 2^30, and >= N without a row_index; hidden and W 16-byte aligned; 1 <= L_max <= 511; reduction 0 or
 * 1.  Anything else: TMI_ERR_INVALID, nothing is launched and nothing written; tmi_last_error names the function and the
 * limits.  tmi_ctc_head_workspace_bytes returns -1 outside the limits.  Values in device memory are never trusted: lengths
 * are clamped and indices checked before use.
 * Not built: a gradient with respect to hidden (the encoder stays frozen), label smoothing. */
int64_t tmi_ctc_head_workspace_bytes(int64_t N, int64_t T_max, int64_t H, int64_t V);
int tmi_ctc_head_fwd(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index,
                     const int32_t* frame_lens, const float* W, const float* b, float p, uint64_t seed, float* logits,
                     int64_t lg_sn, int64_t lg_st, float* logp, int64_t lp_sn, int64_t lp_st, int32_t* argmax, int64_t N,
                     int64_t T_max, int64_t H, int64_t V, void* stream);
int tmi_ctc_head_bwd(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index,
                     const int32_t* frame_lens, const int32_t* label_lens, const float* grad, int64_t gr_sn, int64_t gr_st,
                     const float* nll, const int32_t* infeasible, float p, uint64_t seed, int32_t reduction, float* gW,
                     float* gb, float* loss, int32_t* n_infeasible, void* workspace, int64_t workspace_bytes, int64_t N,
                     int64_t T_max, int64_t L_max, int64_t H, int64_t V, void* stream);

/* ------------------------------------------------------------------------------------
 * The learned weighted sum over encoder layers in front of the CTC head (csrc/layer_mix.hip): the frozen-encoder probe of
 * SUPERB / s3prl (`use_weighted_layer_sum`).  K layers of hidden states, all in x_dtype (TMI_BF16 or TMI_F32) and of one
 * layout: element (s, t, h) of layer k at layers[k][s*x_sn + t*x_st + h].  `layers` is a HOST array of K device pointers; it
 * is copied into the kernels' arguments, so no device-side pointer table exists and the layers may be separate allocations
 * or slices of one stacked [K, n_src, T, H] tensor.  row_index, n_src, frame_lens, the live rows r = n*T_max + t and the
 * clamping of device values are exactly those of tmi_ctc_head_fwd: a dead row is neither read nor written, a row_index entry
 * outside [0, n_src) reads as zeros.  fp32 arithmetic throughout.
 *
 * Both calls form the weights w = softmax(a) from the fp32 logits a [K] in the same way in every workgroup:
 *   m = max_k a[k];  e_k = expf(a[k] - m);  s = e_0 + e_1 + .. in ascending k, starting from e_0;  w_k = e_k / s
 *
 * tmi_layer_mix_fwd, per live row:
 *   mixed[n, t, h] = fmaf(w_k, (float) x_k[s, t, h], acc) for k = 0 .. K-1 in that order, from acc = 0
 * mixed is fp32, element (n, t, h) at mixed[n*m_sn + t*m_st + h], BY POSITION: the gather through row_index happens here, and
 * the head kernels then run on mixed with row_index = NULL and x_dtype = TMI_F32.  w_out fp32 [K] may be NULL; when given it
 * receives w.
 *
 * tmi_layer_mix_bwd: the gradient of loss = sum_n w_n nll[n] with respect to a, from `grad` as tmi_ctc_posteriors wrote it
 * for the log-probs tmi_ctc_head_fwd formed from `mixed` with dropout (p, seed), its infeasible [N], and the head's fp32
 * W [H, V] (contiguous):
 *   w_n       = as tmi_ctc_head_bwd forms it (0 when infeasible[n] != 0: that item's grad is then not read)
 *   gs[r][v]  = grad[r][v] * w_n on a live row
 *   dx[r][h]  = keep(seed, r, h) ? (fmaf(gs[r][v], W[h][v], .) over v = 0 .. V-1 in that order, from 0) * 65536/(65536-thr) : 0
 *               the generator and keying of tmi_ctc_head_fwd: stream 0, row = the position r, column = h, the scale formed
 *               the same way; p == 0 hashes nothing.  dx is never stored to memory.
 *   d_k       = sum over the live rows r and the columns h of dx[r][h] * (float) x_k[s, t, h]                         (*)
 *   g_a[k]    = w_k * (d_k - dot),  dot = fmaf(w_j, d_j, .) over j = 0 .. K-1 in that order, from 0
 *   (*) the rows 0 .. N*T_max - 1 are cut into tiles of tr = 8 * ceil(N*T_max / 8192) consecutive rows (8 rows up to
 *       N*T_max = 8192; at most 1024 tiles).  H is cut into slices of hs = 256 columns (128 when V > 32), a slice into pieces
 *       of 8 consecutive columns; rp = 2048 / hs rows of a tile are in flight at a time.  Thread (j, q) of a tile's 256,
 *       j < rp, q < hs / 8, owns the rows j, j + rp, .. of the tile and in every slice the columns 8 q .. 8 q + 7.  Its sum is
 *       one fmaf chain from 0: the slices in ascending order, inside a slice its rows ascending, inside a row its 8 columns
 *       ascending (a row that is not live, an infeasible item and a piece past H add nothing).  The 64 lanes of a wave -
 *       threads 64 w .. 64 w + 63 in the order (j, q) -> j * (hs / 8) + q - meet in the xor butterfly 32, 16, .., 1; the four
 *       waves are added ((w0 + w1) + w2) + w3: the tile's partial sum.  d_k: lane l of a wave adds the tiles l, l + 64, .. in
 *       ascending order from 0, and the 64 lanes meet in the same butterfly.  The order depends on (N*T_max, H, V) alone.
 * g_a fp32 [K] and, when not NULL, d fp32 [K] (the gradient with respect to the weights themselves) are written, not
 * accumulated; both are zero with no live row.  No floating-point atomic anywhere: the same call gives the same bits.
 * workspace: tmi_layer_mix_workspace_bytes(N, T_max, H, V, K) bytes (the tiles' partial sums, tiles * K floats), 16-byte
 * aligned, any contents.
 *
 * Limits: 1 <= K <= 64; N, T_max, N*T_max, H, V, L_max, p, reduction, the strides (m_st >= H) and n_src as for
 * tmi_ctc_head_*; every layer, mixed and W 16-byte aligned, the other pointers 4.  Anything else, a NULL `layers` or a NULL
 * entry among its first K included: TMI_ERR_INVALID, nothing is launched and nothing written; tmi_last_error names the
 * function and the limits.  tmi_layer_mix_workspace_bytes returns -1 outside the limits.
 * Not built: a LayerNorm per layer before the mix, the same mix in front of the classification head (it needs a gradient with
 * respect to `pooled` that tmi_cls_head_bwd does not form). */
int64_t tmi_layer_mix_workspace_bytes(int64_t N, int64_t T_max, int64_t H, int64_t V, int64_t K);
int tmi_layer_mix_fwd(const void* const* layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                      const int32_t* row_index, const int32_t* frame_lens, const float* a, float* w_out, float* mixed,
                      int64_t m_sn, int64_t m_st, int64_t N, int64_t T_max, int64_t H, void* stream);
int tmi_layer_mix_bwd(const void* const* layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                      const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens, const float* grad,
                      int64_t gr_sn, int64_t gr_st, const int32_t* infeasible, float p, uint64_t seed, int32_t reduction,
                      const float* W, const float* a, float* g_a, float* d, void* workspace, int64_t workspace_bytes, int64_t N,
                      int64_t T_max, int64_t L_max, int64_t H, int64_t V, void* stream);

/* ------------------------------------------------------------------------------------
 * SpecAugment span masks on the probes' cached features (apply_time_mask / apply_feature_mask, V:1073-1119;
 * csrc/spec_augment.hip, and the MASKED instantiations of csrc/ctc_head.hip and csrc/layer_mix.hip).  TensorFlow's RNG stream
 * cannot be reproduced: as at every dropout site the draws are this build's counter-based generator (tmi_keep), the
 * structure is the reference's.
 *   seed      the caller passes the SITE seed: site = (seed + step * 0x9E3779B97F4A7C15 + SITE_SPEC * 0xD1B54A32D192ED03) mod
 *             2^64 with SITE_SPEC = 7 (next to SITE_CTC = 6; the Python layer forms it)
 *   streams   1: the time mask, 2: the feature mask (stream 0 stays the flat dropout's)
 *   start(n, c) = NOT keep[key = the stream's key of (site, stream), row = n, col = c, thr]: tmi_dropout's keep decision and
 *             stream key (csrc/tmi_common.h),  thr = round(prob * 65536) as tmi_dropout forms it;  n = the item's POSITION in
 *             the call;  c = the frame t in [0, T_max) for the time mask, the column h in [0, H) for the feature mask.
 *             prob == 0: no bit is set and nothing is hashed.
 *   mask(n, c)  = OR over i = 0 .. length-1 of start(n, c - i), start false for c - i < 0 (V:1083-1086): a start masks itself
 *             and the length - 1 positions after it, cut at the end of the row.  Starts are drawn over all of T_max whatever
 *             frame_lens says: the mask of frame t does not depend on the clip's length.
 *   effect    a masked element is +0 (V:1092 / V:1117 multiply by 1 - mask): the time mask zeroes whole frames of item n, the
 *             feature mask whole columns of item n, of the tensor the head's Dropout sees (`hidden`, or `mixed` behind a layer
 *             mix; Dropout of a zero is a zero, so the order does not matter).
 *   bits      time_bits uint32 [N][ld_t], ld_t >= ceil(T_max / 32): frame t is bit t % 32 of word t / 32.  feat_bits uint32
 *             [N][ld_f], ld_f >= ceil(H / 32), the same over h.  Bits past T_max / H in the last word are 0; words past
 *             ceil(cols / 32) of a row are not written.
 *
 * tmi_spec_masks draws both bit sets in ONE launch; either pointer may be NULL (that mask is off: its prob, length and ld
 * are not looked at), not both.  counts int32 [N][2] may be NULL; it receives the set bits of each row's time and feature
 * mask (0 for a mask that is off).  Integers only, no atomic: the same call gives the same bits.
 *
 * tmi_span_mask_apply: out = masked ? +0 : x for x [N, T, H] in x_dtype (TMI_BF16 or TMI_F32; element (n, t, h) at
 * x[n*x_sn + t*x_st + h], out the same under o_sn / o_st, in the same dtype; the elements are moved as bits).  Either mask
 * may be NULL.  16-byte accesses when the strides and both pointers allow it, element accesses otherwise.  The probe's step
 * does not use it: it serves apply_time_mask / apply_feature_mask and the unfused comparison.
 *
 * tmi_ctc_head_fwd_m, tmi_ctc_head_bwd_m, tmi_layer_mix_bwd_m take the arguments of tmi_ctc_head_fwd / _bwd /
 * tmi_layer_mix_bwd and (time_bits, ld_t, feat_bits, ld_f), each pointer possibly NULL, BY POSITION n as frame_lens is.
 * They compute what the plain call computes on a copy of hidden (of every layer) with the masked elements of the live rows
 * set to +0, bit for bit: the summation orders, chunks and tiles are the plain call's.  A time-masked live row is not loaded;
 * its xd is zeros, so its logits are b; it still adds its gs to gb, and nothing to gW or d_k.  tmi_layer_mix_bwd_m zeroes dx
 * under the mask where the dropout mask is applied.  tmi_layer_mix_fwd has no masked form: the mix is linear, so masking
 * `mixed` inside the head kernels is masking every layer.  With both pointers NULL each is the plain call.
 *
 * Limits: 1 <= length <= 64; 0 <= prob < 1; N, T_max (T), N*T_max, H as for tmi_ctc_head_*; ld <= 2^30; bit pointers 4-byte
 * aligned.  Anything else: TMI_ERR_INVALID, nothing is launched and nothing written.
 * Not built: HF's min_masks, span counts proportional to the length, masks keyed by the source row, a learned mask
 * embedding, masking in the pre-training step. */
int tmi_spec_masks(uint32_t* time_bits, int64_t ld_t, uint32_t* feat_bits, int64_t ld_f, int32_t* counts, int64_t N, int64_t T_max,
                   int64_t H, float time_prob, int64_t time_length, float feat_prob, int64_t feat_length, uint64_t seed,
                   void* stream);
int tmi_span_mask_apply(const void* x, int32_t x_dtype, int64_t x_sn, int64_t x_st, const uint32_t* time_bits, int64_t ld_t,
                        const uint32_t* feat_bits, int64_t ld_f, void* out, int64_t o_sn, int64_t o_st, int64_t N, int64_t T,
                        int64_t H, void* stream);
int tmi_ctc_head_fwd_m(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index,
                       const int32_t* frame_lens, const float* W, const float* b, float p, uint64_t seed, float* logits,
                       int64_t lg_sn, int64_t lg_st, float* logp, int64_t lp_sn, int64_t lp_st, int32_t* argmax, int64_t N,
                       int64_t T_max, int64_t H, int64_t V, const uint32_t* time_bits, int64_t ld_t, const uint32_t* feat_bits,
                       int64_t ld_f, void* stream);
int tmi_ctc_head_bwd_m(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index,
                       const int32_t* frame_lens, const int32_t* label_lens, const float* grad, int64_t gr_sn, int64_t gr_st,
                       const float* nll, const int32_t* infeasible, float p, uint64_t seed, int32_t reduction, float* gW,
                       float* gb, float* loss, int32_t* n_infeasible, void* workspace, int64_t workspace_bytes, int64_t N,
                       int64_t T_max, int64_t L_max, int64_t H, int64_t V, const uint32_t* time_bits, int64_t ld_t,
                       const uint32_t* feat_bits, int64_t ld_f, void* stream);
int tmi_layer_mix_bwd_m(const void* const* layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                        const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens, const float* grad,
                        int64_t gr_sn, int64_t gr_st, const int32_t* infeasible, float p, uint64_t seed, int32_t reduction,
                        const float* W, const float* a, float* g_a, float* d, void* workspace, int64_t workspace_bytes, int64_t N,
                        int64_t T_max, int64_t L_max, int64_t H, int64_t V, const uint32_t* time_bits, int64_t ld_t,
                        const uint32_t* feat_bits, int64_t ld_f, void* stream);

/* ------------------------------------------------------------------------------------
 * Log-mel front end (speech_jobs/whisper_dist.py:739-766, extract_fbank_features; dead in the
 * reference's training path).  The windowed DFT of the frames is a tmi_gemm
 * (frames = overlapping rows of the waveform, a_sm = hop; B = [n_fft, 2*n_bins] Hann-weighted
 * cos | -sin); this entry turns spec[frames, ld_spec] = [re | im] into
 * log(|X|^2 . mel[n_bins, n_mels] + eps), written frame-major out[f*ld_out + m] (the reference's
 * layout, W:764) or channels-first out[m*ld_out + f] (what the encoder reads).  fp32.
 */
int tmi_logmel_from_spectrum(const float* spec, int64_t ld_spec, const float* mel, float* out,
                             int64_t frames, int32_t n_bins, int32_t n_mels, float eps,
                             int32_t channels_first, int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TETHYS_MI_H */
