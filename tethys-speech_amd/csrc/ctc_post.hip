// CTC forward-backward (Wav2Vec2ForCTC.posteriors): tmi_ctc_posteriors.  include/tethys_mi.h states the contract; this is
// how it is carried out.  All arithmetic is fp32, -inf is the additive zero, no kernel uses an atomic, the only scratch is
// the gamma tensor itself: the same call gives the same bits, and an item gets the bits it gets alone.  Two launches.
//
// ctc_post_kernel - one workgroup per item, thread s owns extended state s of [blank, l1, blank, .., blank], as
//   ctc.hip's ctc_kernel.  The alpha pass IS that kernel's sum semiring, operation for operation (the same lse3 of
//   tmi_common.h): states s - 1 and s - 2 of frame t - 1 arrive by __shfl_up, lanes 62 and 63 of every wave leave theirs in a
//   two-slot LDS pair (s_bnd, slot t & 1), one barrier per frame, the thread's own column of logp prefetched CT_PF frames
//   ahead.  alpha_t(s) is stored to gamma[n][t][s].  ll = LSE3(alpha_{T-1}(S-1), alpha_{T-1}(S-2), -inf) is computed by
//   every thread from the two values in LDS, so nll / infeasible are bit for bit tmi_ctc_forward's.
//   The same workgroup then runs time backwards, t = T-1 .. 0, beta in a register: states s + 1 and s + 2 of frame t + 1
//   arrive by __shfl_down, lanes 0 and 1 of every wave leave theirs in a second two-slot pair (s_top, slot (T-1-t) & 1; the
//   row of a wave that does not exist stays -inf), one barrier per frame; logp and the thread's own alpha (a global read
//   of what this thread wrote) are prefetched CT_PF frames ahead, in reverse.
//     beta_{T-1}(s) = lp[T-1][ext_s] for s = S-1 and, if S > 1, s = S-2; -inf elsewhere
//     beta_t(s)     = lp[t][ext_s] + LSE3(beta_{t+1}(s), beta_{t+1}(s+1), beta_{t+1}(s+2)), the second term only if
//                     s+1 < S, the third only if s+2 < S && ext_{s+2} != blank && ext_{s+2} != ext_s
//     gamma[n,t,s]  = expf((alpha_t(s) - ll) + (beta_t(s) - lp[t][ext_s])): the two differences first, then their sum;
//                     0 whenever alpha_t(s) or beta_t(s) is -inf; not clamped to 1.  It overwrites alpha_t(s).
//     tok_frames[n,i] = sum over t = T-1 down to 0 of gamma[n,t,2i+1], a running fp32 sum from 0 in that order
//     tok_center[n,i] = (sum in the same order of fl(float(t) * gamma[n,t,2i+1]), the product rounded before it is
//                       added) / tok_frames[n,i]
//   An item without a path (ll = -inf): gamma = 0 for t < T, s < S, tok_frames = 0, tok_center = -1; T < 1: the tok_*
//   entries only.  A label length is clamped to [0, L_max], a frame length to T_max, a symbol outside [0, V) is never
//   dereferenced: its log-prob is -inf.
//
// ctc_occ_kernel - grid (frames / OC_ROWS, items), one wave per frame t < T, lane c holds symbol c.  The wave loads 64
//   states of gamma[n][t] and of ext at a time (lane j state s0 + j) and walks them in ascending s by readlane: lane c
//   adds gamma[n,t,s] when ext_s == c.  occ[n,t,c] = that running fp32 sum from 0 (0 for a symbol not in ext),
//   grad[n,t,c] = expf(lp[t][c]) - occ[n,t,c]; for an item without a path (infeasible[n], written by the first launch)
//   occ = grad = 0.  Columns past V and rows past T are not written.
#include "tmi_common.h"
#include <math.h>

namespace {

constexpr int CT_LMAX = 511;   // labels: 2 L + 1 <= 1023 extended states, one thread each
constexpr int CT_TMAX = 4096;  // frames (the limit of tmi_ctc_viterbi: the callers of both share it)
constexpr int CT_PF = 8;       // frames per prefetch
constexpr int CT_WAVES = 1024 / TMI_WAVE;
constexpr int OC_ROWS = 4;     // occupancy: frames (waves) per workgroup

__global__ __launch_bounds__(1024) void ctc_post_kernel(const float* __restrict__ logp, int64_t lp_sn, int64_t lp_st, int V,
                                                        const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ label_lens,
                                                        const int32_t* __restrict__ frame_lens, int blank,
                                                        float* __restrict__ nll, int32_t* __restrict__ infeasible,
                                                        float* gamma, float* __restrict__ tok_frames,
                                                        float* __restrict__ tok_center, int L_max, int T_max,
                                                        int zero_infinity) {
  __shared__ float s_bnd[2][CT_WAVES][2];      // alpha: lanes 62 / 63 of every wave
  __shared__ float s_top[2][CT_WAVES + 1][2];  // beta: lanes 0 / 1 of every wave; row CT_WAVES is never written
  __shared__ float s_fin[2];
  const int n = blockIdx.x;
  int L = label_lens[n], T = frame_lens[n];
  L = L < 0 ? 0 : (L > L_max ? L_max : L);  // (a value outside the contract never leads outside the tensors)
  T = T > T_max ? T_max : T;
  const int S = 2 * L + 1, SW = 2 * L_max + 1;
  const int s = threadIdx.x, lane = s & 63, wv = s >> 6;
  const bool act = s < S;
  const bool tok = act && (s & 1);
  float* __restrict__ tf_out = tok_frames + (int64_t)n * L_max + (s >> 1);
  float* __restrict__ tc_out = tok_center + (int64_t)n * L_max + (s >> 1);
  if (T < 1) {  // (uniform) no frame: no path
    if (s == 0) nll[n] = zero_infinity ? 0.f : INFINITY, infeasible[n] = 1;
    if (tok) *tf_out = 0.f, *tc_out = -1.f;
    return;
  }
  int sym = blank;
  bool skip = false, skipb = false;
  if (tok) {
    sym = labels[(int64_t)n * L_max + (s >> 1)];
    skip = s >= 3 && sym != blank && sym != labels[(int64_t)n * L_max + (s >> 1) - 1];
    if (s + 2 < S) {
      const int nsym = labels[(int64_t)n * L_max + (s >> 1) + 1];
      skipb = nsym != blank && nsym != sym;
    }
  }
  const bool readable = act && sym >= 0 && sym < V;  // (a symbol outside the row is never dereferenced: its log-prob is -inf)
  const float* __restrict__ lp = logp + (int64_t)n * lp_sn + (readable ? sym : 0);
  float* g = gamma + (int64_t)n * T_max * SW + (act ? s : 0);
  if (s < 2 * CT_WAVES * 2) (&s_bnd[0][0][0])[s] = -INFINITY;
  for (int k = s; k < 2 * (CT_WAVES + 1) * 2; k += blockDim.x) (&s_top[0][0][0])[k] = -INFINITY;
  __syncthreads();

  // ---- alpha: ctc.hip's ctc_kernel<false>, plus the store
  float alpha = -INFINITY;
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
          alpha = cur[k] + lse3(alpha, a1, a2);
        }
        if (act) g[(int64_t)t * SW] = alpha;
        if (lane >= 62) s_bnd[t & 1][wv][lane - 62] = alpha;
        __syncthreads();
      }
    }
#pragma unroll
    for (int k = 0; k < CT_PF; ++k) cur[k] = nxt[k];
  }
  if (s == S - 1) s_fin[0] = alpha;
  if (s == S - 2) s_fin[1] = alpha;
  __syncthreads();
  const float last = s_fin[0], lastm1 = S > 1 ? s_fin[1] : -INFINITY;
  const float ll = lse3(last, lastm1, -INFINITY);  // (every thread: the same two values, the same bits)
  const bool ok = ll != -INFINITY;
  if (s == 0) {
    nll[n] = ok ? -ll : (zero_infinity ? 0.f : INFINITY);
    infeasible[n] = ok ? 0 : 1;
  }
  if (!ok) {  // (uniform) no path
    if (act)
      for (int t = 0; t < T; ++t) g[(int64_t)t * SW] = 0.f;
    if (tok) *tf_out = 0.f, *tc_out = -1.f;
    return;
  }

  // ---- beta and gamma, time backwards: step r is frame T - 1 - r
  float beta = -INFINITY, tf = 0.f, tc = 0.f;
  float ca[CT_PF], na[CT_PF];
#pragma unroll
  for (int k = 0; k < CT_PF; ++k) {
    const int t = T - 1 - k;
    cur[k] = (readable && t >= 0) ? lp[(int64_t)t * lp_st] : -INFINITY;
    ca[k] = (act && t >= 0) ? g[(int64_t)t * SW] : -INFINITY;
  }
  for (int r0 = 0; r0 < T; r0 += CT_PF) {
#pragma unroll
    for (int k = 0; k < CT_PF; ++k) {
      const int t = T - 1 - (r0 + CT_PF + k);
      nxt[k] = (readable && t >= 0) ? lp[(int64_t)t * lp_st] : -INFINITY;
      na[k] = (act && t >= 0) ? g[(int64_t)t * SW] : -INFINITY;
    }
#pragma unroll
    for (int k = 0; k < CT_PF; ++k) {
      const int r = r0 + k;
      if (r < T) {  // (uniform)
        const int t = T - 1 - r;
        float b1 = __shfl_down(beta, 1, 64), b2 = __shfl_down(beta, 2, 64);
        if (lane >= 62) {
          const float u0 = s_top[(r + 1) & 1][wv + 1][0];  // lane 0 of the wave above (-inf where there is none)
          const float u1 = s_top[(r + 1) & 1][wv + 1][1];  // lane 1
          b2 = lane == 63 ? u1 : u0;
          b1 = lane == 63 ? u0 : b1;
        }
        if (!skipb) b2 = -INFINITY;  // (a thread past S - 1 holds -inf: the second term needs no flag)
        if (r == 0) {
          beta = (act && s >= S - 2) ? cur[k] : -INFINITY;
        } else if (act) {
          beta = cur[k] + lse3(beta, b1, b2);
        }
        if (lane < 2) s_top[r & 1][wv][lane] = beta;
        float gm = 0.f;
        if (act) {
          if (ca[k] != -INFINITY && beta != -INFINITY) gm = expf((ca[k] - ll) + (beta - cur[k]));
          g[(int64_t)t * SW] = gm;
        }
        tf += gm;
        tc += __fmul_rn((float)t, gm);
        __syncthreads();
      }
    }
#pragma unroll
    for (int k = 0; k < CT_PF; ++k) cur[k] = nxt[k], ca[k] = na[k];
  }
  if (tok) *tf_out = tf, *tc_out = tc / tf;
}

__global__ __launch_bounds__(OC_ROWS * TMI_WAVE) void ctc_occ_kernel(const float* __restrict__ logp, int64_t lp_sn,
                                                                    int64_t lp_st, int V, const int32_t* __restrict__ labels,
                                                                    const int32_t* __restrict__ label_lens,
                                                                    const int32_t* __restrict__ frame_lens, int blank,
                                                                    const int32_t* __restrict__ infeasible,
                                                                    const float* __restrict__ gamma, float* __restrict__ occ,
                                                                    int64_t oc_sn, int64_t oc_st, float* __restrict__ grad,
                                                                    int64_t gr_sn, int64_t gr_st, int L_max, int T_max) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int t = blockIdx.x * OC_ROWS + (threadIdx.x >> 6);
  int L = label_lens[n], T = frame_lens[n];
  L = L < 0 ? 0 : (L > L_max ? L_max : L);
  T = T > T_max ? T_max : T;
  if (t >= T) return;  // (uniform over the wave)
  const int S = 2 * L + 1, SW = 2 * L_max + 1;
  const bool ok = infeasible[n] == 0;
  const float* __restrict__ gm = gamma + ((int64_t)n * T_max + t) * SW;
  const int32_t* __restrict__ lab = labels + (int64_t)n * L_max;
  float acc = 0.f;
  if (ok) {
    for (int s0 = 0; s0 < S; s0 += 64) {
      const int sx = s0 + lane;
      float gv = 0.f;
      int ev = -1;
      if (sx < S) {
        gv = gm[sx];
        ev = (sx & 1) ? lab[sx >> 1] : blank;
      }
      const int cnt = S - s0 < 64 ? S - s0 : 64;
      for (int j = 0; j < cnt; ++j) {  // ascending s
        const float gj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gv), j));
        const int ej = __builtin_amdgcn_readlane(ev, j);
        acc += ej == lane ? gj : 0.f;
      }
    }
  }
  if (lane < V) {
    occ[(int64_t)n * oc_sn + (int64_t)t * oc_st + lane] = acc;
    if (grad != nullptr)
      grad[(int64_t)n * gr_sn + (int64_t)t * gr_st + lane] =
          ok ? expf(logp[(int64_t)n * lp_sn + (int64_t)t * lp_st + lane]) - acc : 0.f;
  }
}

unsigned ctc_threads(int64_t L_max) { return (unsigned)((2 * L_max + 1 + TMI_WAVE - 1) / TMI_WAVE * TMI_WAVE); }

}  // namespace

static int tmi_ctc_posteriors_impl(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* labels,
                                   const int32_t* label_lens, const int32_t* frame_lens, int32_t blank, float* nll,
                                   int32_t* infeasible, float* gamma, float* occ, int64_t oc_sn, int64_t oc_st, float* grad,
                                   int64_t gr_sn, int64_t gr_st, float* tok_frames, float* tok_center, int64_t N, int64_t L_max,
                                   int64_t T_max, int32_t zero_infinity, void* stream) {
  const int64_t lim = (int64_t)1 << 30;
  const bool sizes = N >= 1 && N <= 65535 && L_max >= 1 && L_max <= CT_LMAX && T_max >= 1 && T_max <= CT_TMAX && V >= 2 && V <= 64;
  const bool ptrs = logp && labels && label_lens && frame_lens && nll && infeasible && gamma && occ && tok_frames && tok_center &&
                    tmi_aligned(logp, 4) && tmi_aligned(labels, 4) && tmi_aligned(label_lens, 4) && tmi_aligned(frame_lens, 4) && tmi_aligned(nll, 4) && tmi_aligned(infeasible, 4) &&
                    tmi_aligned(gamma, 4) && tmi_aligned(occ, 4) && tmi_aligned(grad, 4) && tmi_aligned(tok_frames, 4) && tmi_aligned(tok_center, 4);
  const bool strides = sizes && blank >= 0 && blank < V && lp_st >= V && lp_st <= lim && lp_sn >= T_max * lp_st && oc_st >= V &&
                       oc_st <= lim && oc_sn >= T_max * oc_st &&
                       (grad == nullptr || (gr_st >= V && gr_st <= lim && gr_sn >= T_max * gr_st));
  if (!sizes || !ptrs || !strides || (zero_infinity != 0 && zero_infinity != 1)) {
    tmi_set_error("tmi_ctc_posteriors: bad argument (non-NULL 4-byte aligned pointers, grad may be NULL; 1 <= N <= 65535 items, "
                  "one workgroup each; 1 <= L_max <= 511 labels, one thread per extended state; 1 <= T_max <= 4096 frames; "
                  "2 <= V <= 64 symbols, one lane each; 0 <= blank < V; V <= lp_st <= 2^30, lp_sn >= T_max lp_st, and the same for "
                  "oc_st / oc_sn and gr_st / gr_sn; zero_infinity 0 / 1)");
    return TMI_ERR_INVALID;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ctc_post_kernel, dim3((unsigned)N), dim3(ctc_threads(L_max)), 0, st, logp, lp_sn, lp_st, (int)V, labels,
                     label_lens, frame_lens, (int)blank, nll, infeasible, gamma, tok_frames, tok_center, (int)L_max, (int)T_max,
                     (int)zero_infinity);
  const int rc = tmi_check_launch("tmi_ctc_posteriors");
  if (rc != 0) return rc;
  hipLaunchKernelGGL(ctc_occ_kernel, dim3((unsigned)((T_max + OC_ROWS - 1) / OC_ROWS), (unsigned)N), dim3(OC_ROWS * TMI_WAVE), 0, st,
                     logp, lp_sn, lp_st, (int)V, labels, label_lens, frame_lens, (int)blank, infeasible, gamma, occ, oc_sn, oc_st,
                     grad, gr_sn, gr_st, (int)L_max, (int)T_max);
  return tmi_check_launch("tmi_ctc_posteriors");
}

extern "C" int tmi_ctc_posteriors(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* labels,
                                  const int32_t* label_lens, const int32_t* frame_lens, int32_t blank, float* nll,
                                  int32_t* infeasible, float* gamma, float* occ, int64_t oc_sn, int64_t oc_st, float* grad,
                                  int64_t gr_sn, int64_t gr_st, float* tok_frames, float* tok_center, int64_t N, int64_t L_max,
                                  int64_t T_max, int32_t zero_infinity, void* stream) {
  return tmi_plan_run<tmi_ctc_posteriors_impl>(logp, lp_sn, lp_st, V, labels, label_lens, frame_lens, blank, nll, infeasible,
                                               gamma, occ, oc_sn, oc_st, grad, gr_sn, gr_st, tok_frames, tok_center, N, L_max,
                                               T_max, zero_infinity, stream);
}
