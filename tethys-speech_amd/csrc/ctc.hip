// CTC inference (Wav2Vec2ForCTC): tmi_ctc_logsoftmax, tmi_ctc_greedy, tmi_ctc_forward and tmi_ctc_viterbi.
// include/tethys_mi.h states the contracts; this is how they are carried out.  All arithmetic is fp32, -inf is the
// additive zero, no kernel uses an atomic: the same call gives the same bits.
//
// tmi_ctc_logsoftmax - one wave per row, lane l holds column l (V <= 64; a lane past V holds -inf and is never loaded
//   or stored).  m = the wave maximum (exact), e = expf(x - m), the sum is the butterfly of wave_sum (lane distance 32,
//   16, .., 1), lse = m + logf(sum), logp = x - lse.  argmax = the lowest lane whose x equals m (a ballot).
//
// tmi_ctc_greedy - one workgroup of 256 threads per item, a chunk of 256 consecutive frames at a time, frame t on thread
//   t & 255.  A frame emits when a[t] != blank and (t == 0 or a[t] != a[t-1]); a frame ENDS a run when a[t] != blank and
//   (t == len - 1 or a[t+1] != a[t]).  Every non-blank run has one of each, the start not after the end, so with
//   E(t) = the number of emitting frames <= t the start writes entry E(t) - 1 and so does the end.  E(t) = the chunks
//   before (a running count) + the waves before in this chunk (LDS, four words) + popcount(ballot & lanes <= mine).
//   best_logprob: thread i adds logp[t][a[t]] for t = i, i + 256, .. in ascending t, then wave_sum's butterfly, then
//   the four wave sums ((w0 + w1) + w2) + w3.
//
// tmi_ctc_forward / tmi_ctc_viterbi - ONE kernel body (ctc_kernel<VIT>), two semirings.  One workgroup per item, thread
//   s owns extended state s of [blank, l1, blank, .., blank]; alpha lives in a register.  At frame t the values of
//   states s - 1 and s - 2 of frame t - 1 arrive by lane shuffles; across a wave seam lanes 62 and 63 of every wave
//   leave theirs in a two-slot LDS pair (slot t & 1), so ONE barrier per frame orders the read of the previous frame's
//   slot and the write of this frame's - tmi_dtw's s_bnd.  A thread reads one column of logp (its own symbol) frame
//   after frame: every lane of the workgroup is on the same one or two cache lines, the CT_PF frames after the current
//   CT_PF are loaded while those are computed.  Sum semiring: m = max of the candidates, m + logf((e0 + e1) + e2) with
//   e_i = expf(a_i - m) (an absent candidate is -inf: its e is 0), -inf when m is.  Max semiring: the candidates in
//   the order stay, step, skip, a later one wins only when strictly larger; the move goes, 2 bits per (frame, state)
//   and 16 frames to a word, to workspace[(n * ceil(T_max / 16) + t / 16) * (2 L_max + 1) + s] - the threads of a
//   workgroup write neighbouring words.  The walk back: the workgroup stages CT_ROWS word rows (16 frames each) in LDS,
//   thread 0 walks them from the last frame down and writes states and token bounds itself.
#include "tmi_common.h"
#include <math.h>

namespace {

constexpr int LS_ROWS = 4;       // log-softmax: rows (waves) per workgroup
constexpr int GR_THREADS = 256;  // greedy: frames per chunk
constexpr int CT_LMAX = 511;     // labels: 2 L + 1 <= 1023 extended states, one thread each
constexpr int CT_TMAX = 4096;    // Viterbi: frames (the moves of CT_ROWS * 16 frames are staged in LDS)
constexpr int CT_PF = 8;         // frames per log-prob prefetch
constexpr int CT_ROWS = 8;       // word rows per piece of the walk back

__global__ __launch_bounds__(LS_ROWS * TMI_WAVE) void ctc_logsoftmax_kernel(const float* __restrict__ x, int64_t ld,
                                                                           int R, int V, float* __restrict__ y,
                                                                           int64_t lp_ld, int32_t* __restrict__ amax) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * LS_ROWS + (threadIdx.x >> 6);
  if (r >= R) return;  // (uniform over the wave)
  const bool in = lane < V;
  const float v = in ? x[r * ld + lane] : -INFINITY;
  const float m = wave_max(v);
  const float e = in ? expf(v - m) : 0.f;  // (m is -inf only when every entry is: the row is then NaN, as the definition gives)
  const float lse = m + logf(wave_sum(e));
  if (in) y[r * lp_ld + lane] = v - lse;
  const unsigned long long eq = __ballot(in && v == m);
  if (lane == 0) amax[r] = eq ? (int32_t)__builtin_ctzll(eq) : 0;
}

__global__ __launch_bounds__(GR_THREADS) void ctc_greedy_kernel(const int32_t* __restrict__ amax,
                                                               const float* __restrict__ logp, int64_t lp_ld,
                                                               const int32_t* __restrict__ frame_lens, int blank,
                                                               int32_t* __restrict__ tokens, int32_t* __restrict__ out_len,
                                                               int32_t* __restrict__ tok_start, int32_t* __restrict__ tok_end,
                                                               float* __restrict__ best, int T_max) {
  __shared__ int s_cnt[2][GR_THREADS / TMI_WAVE];
  __shared__ float s_sum[GR_THREADS / TMI_WAVE];
  const int n = blockIdx.x;
  int len = frame_lens[n];
  len = len > T_max ? T_max : len;
  if (len < 1) return;  // (uniform: the item is skipped entirely)
  const int i = threadIdx.x, lane = i & 63, wv = i >> 6;
  const int32_t* __restrict__ an = amax + (int64_t)n * T_max;
  const float* __restrict__ ln = logp + (int64_t)n * T_max * lp_ld;
  const int64_t o = (int64_t)n * T_max;
  int base = 0;  // emitting frames of the chunks before
  float acc = 0.f;
  for (int t0 = 0, it = 0; t0 < len; t0 += GR_THREADS, ++it) {  // (every thread runs every chunk: ballots and barriers are uniform)
    const int t = t0 + i;
    const bool live = t < len;
    const int a = live ? an[t] : blank;
    const int prev = (live && t > 0) ? an[t - 1] : -1;
    const int next = (live && t + 1 < len) ? an[t + 1] : -1;
    const bool emit = live && a != blank && (t == 0 || a != prev);
    const bool ends = live && a != blank && (t + 1 == len || a != next);
    if (live && a >= 0 && a < lp_ld) acc += ln[(int64_t)t * lp_ld + a];
    const unsigned long long bal = __ballot(emit);
    if (lane == 0) s_cnt[it & 1][wv] = __popcll(bal);
    __syncthreads();  // (two slots: the next chunk's write cannot overtake this chunk's reads)
    int before = base, all = 0;
#pragma unroll
    for (int w = 0; w < GR_THREADS / TMI_WAVE; ++w) {
      const int c = s_cnt[it & 1][w];
      before += w < wv ? c : 0;
      all += c;
    }
    const int upto = before + __popcll(bal & (~0ull >> (63 - lane)));  // E(t)
    if (emit) {
      tokens[o + upto - 1] = a;
      tok_start[o + upto - 1] = t;
    }
    if (ends) tok_end[o + upto - 1] = t + 1;
    base += all;
  }
  acc = wave_sum(acc);
  if (lane == 0) s_sum[wv] = acc;
  __syncthreads();
  if (i == 0) {
    out_len[n] = base;
    best[n] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
  }
}

// The walk back of the max semiring; every thread of the workgroup calls it, thread 0 walks.
__device__ __forceinline__ void ctc_walk_back(const uint32_t* ws_n, int SW, int S, int T, int L, int end_state, bool feasible,
                                              int32_t* __restrict__ ts, int32_t* __restrict__ te, int32_t* __restrict__ st) {
  __shared__ uint32_t s_mv[CT_ROWS][2 * CT_LMAX + 1];
  const int i = threadIdx.x;
  if (!feasible) {  // (uniform)
    for (int k = i; k < L; k += blockDim.x) ts[k] = -1, te[k] = -1;
    if (st != nullptr)
      for (int k = i; k < T; k += blockDim.x) st[k] = -1;
    return;
  }
  int s = end_state, last = -1;  // (thread 0's)
  for (int r_hi = (T - 1) >> 4; r_hi >= 0; r_hi -= CT_ROWS) {
    const int r_lo = r_hi - CT_ROWS + 1 > 0 ? r_hi - CT_ROWS + 1 : 0;
    for (int r = r_lo; r <= r_hi; ++r)
      if (i < S) s_mv[r - r_lo][i] = ws_n[(int64_t)r * SW + i];
    __syncthreads();
    if (i == 0) {
      const int t_hi = r_hi * 16 + 15 < T - 1 ? r_hi * 16 + 15 : T - 1;
      for (int t = t_hi; t >= r_lo * 16; --t) {
        if (st != nullptr) st[t] = s;
        if (s & 1) {
          if (s != last) te[s >> 1] = t + 1;
          ts[s >> 1] = t;
        }
        last = s;
        if (t > 0) {
          const int mv = (int)((s_mv[(t >> 4) - r_lo][s] >> (2 * (t & 15))) & 3u);
          s -= mv < s ? mv : s;  // (a finite total has a genuine move in every cell of its path; the walk stays inside the states)
        }
      }
    }
    __syncthreads();
  }
}

template <bool VIT>
__global__ __launch_bounds__(1024) void ctc_kernel(const float* __restrict__ logp, int64_t lp_sn, int64_t lp_st,
                                                   const int32_t* __restrict__ labels, const int32_t* __restrict__ label_lens,
                                                   const int32_t* __restrict__ frame_lens, int blank, float* __restrict__ out,
                                                   int32_t* __restrict__ infeasible, int L_max, int T_max, int zero_infinity,
                                                   int32_t* __restrict__ tok_start, int32_t* __restrict__ tok_end,
                                                   int32_t* __restrict__ states, uint32_t* moves_ws) {
  __shared__ float s_bnd[2][1024 / TMI_WAVE][2];
  __shared__ float s_fin[2];
  const int n = blockIdx.x;
  int L = label_lens[n], T = frame_lens[n];
  L = L < 0 ? 0 : (L > L_max ? L_max : L);  // (a value outside the contract never leads outside the tensors)
  T = T > T_max ? T_max : T;
  const int S = 2 * L + 1, SW = 2 * L_max + 1;
  const int s = threadIdx.x, lane = s & 63, wv = s >> 6;
  if (T < 1) {  // (uniform) no frame: no path
    if (s == 0) out[n] = VIT ? -INFINITY : (zero_infinity ? 0.f : INFINITY), infeasible[n] = 1;
    if constexpr (VIT) ctc_walk_back(nullptr, SW, S, 0, L, 0, false, tok_start + (int64_t)n * L_max, tok_end + (int64_t)n * L_max, nullptr);
    return;
  }
  const bool act = s < S;
  int sym = blank;
  bool skip = false;
  if (act && (s & 1)) {
    sym = labels[(int64_t)n * L_max + (s >> 1)];
    skip = s >= 3 && sym != blank && sym != labels[(int64_t)n * L_max + (s >> 1) - 1];
  }
  const bool readable = act && sym >= 0 && sym < lp_st;  // (a symbol outside the row is never dereferenced: its log-prob is -inf)
  const float* __restrict__ lp = logp + (int64_t)n * lp_sn + (readable ? sym : 0);
  const int wpr = (T_max + 15) >> 4;
  uint32_t* mi = VIT ? moves_ws + (int64_t)n * wpr * SW + (act ? s : 0) : nullptr;
  if (s < 2 * (1024 / TMI_WAVE) * 2) (&s_bnd[0][0][0])[s] = -INFINITY;
  __syncthreads();

  float alpha = -INFINITY;
  uint32_t word = 0u;
  float cur[CT_PF], nxt[CT_PF];
#pragma unroll
  for (int k = 0; k < CT_PF; ++k) cur[k] = (readable && k < T) ? lp[(int64_t)k * lp_st] : -INFINITY;
  for (int t0 = 0; t0 < T; t0 += CT_PF) {  // (every thread runs every frame: the barriers and shuffles are uniform)
#pragma unroll
    for (int k = 0; k < CT_PF; ++k) {
      const int t = t0 + CT_PF + k;
      nxt[k] = (readable && t < T) ? lp[(int64_t)t * lp_st] : -INFINITY;
    }
#pragma unroll
    for (int k = 0; k < CT_PF; ++k) {
      const int t = t0 + k;
      if (t < T) {  // (uniform)
        float a1 = __shfl_up(alpha, 1, 64), a2 = __shfl_up(alpha, 2, 64);
        if (lane < 2) {
          const float b0 = wv > 0 ? s_bnd[(t + 1) & 1][wv - 1][0] : -INFINITY;  // lane 62 of the wave below
          const float b1 = wv > 0 ? s_bnd[(t + 1) & 1][wv - 1][1] : -INFINITY;  // lane 63
          a2 = lane == 0 ? b0 : b1;
          a1 = lane == 0 ? b1 : a1;
        }
        if (!skip) a2 = -INFINITY;
        if (t == 0) {
          alpha = (act && s < 2) ? cur[k] : -INFINITY;
        } else if (act) {
          if constexpr (VIT) {
            float b = alpha;
            uint32_t mv = 0u;
            if (a1 > b) b = a1, mv = 1u;
            if (a2 > b) b = a2, mv = 2u;
            alpha = cur[k] + b;
            word |= mv << (2 * (t & 15));
          } else {
            alpha = cur[k] + lse3(alpha, a1, a2);
          }
        }
        if constexpr (VIT) {
          if (act && ((t & 15) == 15 || t == T - 1)) {
            mi[(int64_t)(t >> 4) * SW] = word;
            word = 0u;
          }
        }
        if (lane >= 62) s_bnd[t & 1][wv][lane - 62] = alpha;
        __syncthreads();
      }
    }
#pragma unroll
    for (int k = 0; k < CT_PF; ++k) cur[k] = nxt[k];
  }
  if (s == S - 1) s_fin[0] = alpha;
  if (s == S - 2) s_fin[1] = alpha;
  if constexpr (VIT) __threadfence_block();  // the move words of every state, before the walk back reads them
  __syncthreads();
  const float last = s_fin[0], lastm1 = S > 1 ? s_fin[1] : -INFINITY;
  if constexpr (VIT) {
    const bool pen = lastm1 > last;
    const float tot = pen ? lastm1 : last;
    const bool ok = tot != -INFINITY;
    if (s == 0) out[n] = tot, infeasible[n] = ok ? 0 : 1;
    ctc_walk_back(moves_ws + (int64_t)n * wpr * SW, SW, S, T, L, pen ? S - 2 : S - 1, ok, tok_start + (int64_t)n * L_max,
                  tok_end + (int64_t)n * L_max, states ? states + (int64_t)n * T_max : nullptr);
  } else if (s == 0) {
    const float ll = lse3(last, lastm1, -INFINITY);
    const bool ok = ll != -INFINITY;
    out[n] = ok ? -ll : (zero_infinity ? 0.f : INFINITY);
    infeasible[n] = ok ? 0 : 1;
  }
}

bool ctc_common_ok(const float* logp, int64_t lp_sn, int64_t lp_st, const int32_t* labels, const int32_t* label_lens,
                   const int32_t* frame_lens, int32_t blank, const void* out, const int32_t* infeasible, int64_t N,
                   int64_t L_max, int64_t T_max, int64_t t_lim) {
  return logp && labels && label_lens && frame_lens && out && infeasible && tmi_aligned(logp, 4) && tmi_aligned(labels, 4) &&
         tmi_aligned(label_lens, 4) && tmi_aligned(frame_lens, 4) && tmi_aligned(out, 4) && tmi_aligned(infeasible, 4) && N >= 1 && N <= 65535 && L_max >= 1 &&
         L_max <= CT_LMAX && T_max >= 1 && T_max <= t_lim && lp_st >= 1 && lp_st <= ((int64_t)1 << 30) &&
         lp_sn >= T_max * lp_st && blank >= 0 && blank < lp_st;
}

unsigned ctc_threads(int64_t L_max) { return (unsigned)((2 * L_max + 1 + TMI_WAVE - 1) / TMI_WAVE * TMI_WAVE); }

}  // namespace

static int tmi_ctc_logsoftmax_impl(const float* logits, int64_t ld, int64_t R, int64_t V, float* logp, int64_t lp_ld,
                                   int32_t* argmax, void* stream) {
  const int64_t lim = (int64_t)1 << 30;
  if (!logits || !logp || !argmax || !tmi_aligned(logits, 4) || !tmi_aligned(logp, 4) || !tmi_aligned(argmax, 4) || R < 1 || R > lim || V < 2 || V > 64 ||
      ld < V || ld > lim || lp_ld < V || lp_ld > lim) {
    tmi_set_error("tmi_ctc_logsoftmax: bad argument (non-NULL 4-byte aligned pointers; 1 <= R <= 2^30 rows; 2 <= V <= 64 "
                  "columns, one lane each; ld >= V, lp_ld >= V)");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(ctc_logsoftmax_kernel, dim3((unsigned)((R + LS_ROWS - 1) / LS_ROWS)), dim3(LS_ROWS * TMI_WAVE), 0,
                     reinterpret_cast<hipStream_t>(stream), logits, ld, (int)R, (int)V, logp, lp_ld, argmax);
  return tmi_check_launch("tmi_ctc_logsoftmax");
}

extern "C" int tmi_ctc_logsoftmax(const float* logits, int64_t ld, int64_t R, int64_t V, float* logp, int64_t lp_ld,
                                  int32_t* argmax, void* stream) {
  return tmi_plan_run<tmi_ctc_logsoftmax_impl>(logits, ld, R, V, logp, lp_ld, argmax, stream);
}

static int tmi_ctc_greedy_impl(const int32_t* argmax, const float* logp, int64_t lp_ld, const int32_t* frame_lens,
                               int32_t blank, int32_t* tokens, int32_t* out_len, int32_t* tok_start, int32_t* tok_end,
                               float* best_logprob, int64_t N, int64_t T_max, void* stream) {
  if (!argmax || !logp || !frame_lens || !tokens || !out_len || !tok_start || !tok_end || !best_logprob || !tmi_aligned(argmax, 4) ||
      !tmi_aligned(logp, 4) || !tmi_aligned(frame_lens, 4) || !tmi_aligned(tokens, 4) || !tmi_aligned(out_len, 4) || !tmi_aligned(tok_start, 4) || !tmi_aligned(tok_end, 4) ||
      !tmi_aligned(best_logprob, 4) || N < 1 || N > 65535 || T_max < 1 || T_max > ((int64_t)1 << 30) || lp_ld < 1 ||
      lp_ld > ((int64_t)1 << 30) || blank < 0) {
    tmi_set_error("tmi_ctc_greedy: bad argument (non-NULL 4-byte aligned pointers; 1 <= N <= 65535 items, one workgroup "
                  "each; 1 <= T_max <= 2^30 frames; 1 <= lp_ld <= 2^30; blank >= 0)");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(ctc_greedy_kernel, dim3((unsigned)N), dim3(GR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), argmax,
                     logp, lp_ld, frame_lens, (int)blank, tokens, out_len, tok_start, tok_end, best_logprob, (int)T_max);
  return tmi_check_launch("tmi_ctc_greedy");
}

extern "C" int tmi_ctc_greedy(const int32_t* argmax, const float* logp, int64_t lp_ld, const int32_t* frame_lens,
                              int32_t blank, int32_t* tokens, int32_t* out_len, int32_t* tok_start, int32_t* tok_end,
                              float* best_logprob, int64_t N, int64_t T_max, void* stream) {
  return tmi_plan_run<tmi_ctc_greedy_impl>(argmax, logp, lp_ld, frame_lens, blank, tokens, out_len, tok_start, tok_end,
                                           best_logprob, N, T_max, stream);
}

static int tmi_ctc_forward_impl(const float* logp, int64_t lp_sn, int64_t lp_st, const int32_t* labels,
                                const int32_t* label_lens, const int32_t* frame_lens, int32_t blank, float* nll,
                                int32_t* infeasible, int64_t N, int64_t L_max, int64_t T_max, int32_t zero_infinity,
                                void* stream) {
  if (!ctc_common_ok(logp, lp_sn, lp_st, labels, label_lens, frame_lens, blank, nll, infeasible, N, L_max, T_max,
                     (int64_t)INT32_MAX - 2 * CT_PF) ||
      (zero_infinity != 0 && zero_infinity != 1)) {
    tmi_set_error("tmi_ctc_forward: bad argument (non-NULL 4-byte aligned pointers; 1 <= N <= 65535 items, one workgroup "
                  "each; 1 <= L_max <= 511 labels, one thread per extended state; 1 <= T_max <= 2^31 - 17; 1 <= lp_st <= 2^30, "
                  "lp_sn >= T_max lp_st; 0 <= blank < lp_st; zero_infinity 0 / 1)");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(ctc_kernel<false>, dim3((unsigned)N), dim3(ctc_threads(L_max)), 0, reinterpret_cast<hipStream_t>(stream),
                     logp, lp_sn, lp_st, labels, label_lens, frame_lens, (int)blank, nll, infeasible, (int)L_max, (int)T_max,
                     (int)zero_infinity, nullptr, nullptr, nullptr, nullptr);
  return tmi_check_launch("tmi_ctc_forward");
}

extern "C" int tmi_ctc_forward(const float* logp, int64_t lp_sn, int64_t lp_st, const int32_t* labels, const int32_t* label_lens,
                               const int32_t* frame_lens, int32_t blank, float* nll, int32_t* infeasible, int64_t N,
                               int64_t L_max, int64_t T_max, int32_t zero_infinity, void* stream) {
  return tmi_plan_run<tmi_ctc_forward_impl>(logp, lp_sn, lp_st, labels, label_lens, frame_lens, blank, nll, infeasible, N, L_max,
                                            T_max, zero_infinity, stream);
}

extern "C" int64_t tmi_ctc_workspace_bytes(int64_t N, int64_t L_max, int64_t T_max) {
  if (N < 1 || N > 65535 || L_max < 1 || L_max > CT_LMAX || T_max < 1 || T_max > CT_TMAX) return -1;
  return N * ((T_max + 15) / 16) * (2 * L_max + 1) * (int64_t)sizeof(uint32_t);
}

static int tmi_ctc_viterbi_impl(const float* logp, int64_t lp_sn, int64_t lp_st, const int32_t* labels,
                                const int32_t* label_lens, const int32_t* frame_lens, int32_t blank, int32_t* tok_start,
                                int32_t* tok_end, float* total, int32_t* states, int32_t* infeasible, int64_t N, int64_t L_max,
                                int64_t T_max, void* workspace, int64_t workspace_bytes, void* stream) {
  const int64_t need = tmi_ctc_workspace_bytes(N, L_max, T_max);
  if (!ctc_common_ok(logp, lp_sn, lp_st, labels, label_lens, frame_lens, blank, total, infeasible, N, L_max, T_max, CT_TMAX) ||
      !tok_start || !tok_end || !workspace || !tmi_aligned(tok_start, 4) || !tmi_aligned(tok_end, 4) || !tmi_aligned(states, 4) || !tmi_aligned(workspace, 4) ||
      need < 0 || workspace_bytes < need) {
    tmi_set_error("tmi_ctc_viterbi: bad argument (non-NULL 4-byte aligned pointers, states may be NULL; 1 <= N <= 65535 items, "
                  "one workgroup each; 1 <= L_max <= 511 labels; 1 <= T_max <= 4096 frames; 1 <= lp_st <= 2^30, lp_sn >= T_max "
                  "lp_st; 0 <= blank < lp_st; workspace of tmi_ctc_workspace_bytes)");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(ctc_kernel<true>, dim3((unsigned)N), dim3(ctc_threads(L_max)), 0, reinterpret_cast<hipStream_t>(stream),
                     logp, lp_sn, lp_st, labels, label_lens, frame_lens, (int)blank, total, infeasible, (int)L_max, (int)T_max, 0,
                     tok_start, tok_end, states, reinterpret_cast<uint32_t*>(workspace));
  return tmi_check_launch("tmi_ctc_viterbi");
}

extern "C" int tmi_ctc_viterbi(const float* logp, int64_t lp_sn, int64_t lp_st, const int32_t* labels, const int32_t* label_lens,
                               const int32_t* frame_lens, int32_t blank, int32_t* tok_start, int32_t* tok_end, float* total,
                               int32_t* states, int32_t* infeasible, int64_t N, int64_t L_max, int64_t T_max, void* workspace,
                               int64_t workspace_bytes, void* stream) {
  return tmi_plan_run<tmi_ctc_viterbi_impl>(logp, lp_sn, lp_st, labels, label_lens, frame_lens, blank, tok_start, tok_end, total,
                                            states, infeasible, N, L_max, T_max, workspace, workspace_bytes, stream);
}
