// CTC prefix beam search (Wav2Vec2ForCTC.decode(num_beams=K)): tmi_ctc_beam.  include/tethys_mi.h states the contract; this
// is how it is carried out.  All arithmetic is fp32, -inf is the additive zero, no atomics: the same call gives the same
// bits, and an item computes the same bits whatever the batch around it.
//
// One workgroup of K waves per item: wave k holds beam k (pb, pnb, the last token, the length, its trie node and its
// parent's, a hash of the sequence - the same values in every lane), lane c holds symbol c.  Lane `blank` of wave k owns
// the stay candidate of beam k, lane c != blank the extension by c, so the K (V - 1) + K candidates sit one per thread.
//
// A frame:
//   1. every lane reads lp[t][c] (the CB_PF frames after the current CB_PF are loaded while those are computed; every wave
//      is on the same one or two cache lines), lp[blank] and lp[e] come by lane shuffles.  An extension looks for its
//      sequence among the beams of the set (records in LDS): the last token, the length and the hash filter, then the two
//      trie chains are walked back until they meet in one node (equal) or two tokens differ - the node ids alone do not
//      decide, a prefix that left the set and was created again has a second node.  A match leaves v in s_fold[p].
//      The walk reads records of earlier frames only (the beam's own comes from its registers), so a frame's trie stores
//      need not be complete before the next frame's barrier.
//   2. barrier.  The stay lane folds s_fold[k] into pnb', resets the slot and takes score = LSE2(pb', pnb'); an extension's
//      score is v.  Candidates become 64-bit keys (the score's bits made monotone, then ~(ext, k, c): the larger key is
//      the larger score, among equal scores the lower candidate index; 0 = none or -inf) and each wave's maximum goes to
//      s_head.
//   3. barrier, then up to K rounds, one barrier each: every wave reads the K heads and finds the same winner; the winner's
//      lane writes rank r's record (an extension takes the trie node 1 + t K + r), its wave takes the maximum of what it
//      has left, and the heads go to the other slot.  A round whose winner is 0 ends the frame: -inf candidates are
//      never kept.  Wave r then loads rank r's record and stores its node (parent node, token) if the frame created it.
//      The maxima are DPP row rotations and scalar reads, no LDS traffic.
// After the last frame lane 0 of wave r walks rank r's chain back into tokens[n][r][len-1 .. 0].
//
// tmi_ctc_beam_lm is the same kernel with the compile-time flag LM set (tmi_ctc_beam is the instantiation without it: the
// record, the loads and the arithmetic it had).  A beam then also carries g (the weighted LM terms of its tokens, summed in
// token order) and ctx (its last order - 1 tokens as base-V digits, the row of the table its extensions read).  Lane c of
// wave k loads lm[ctx V + c] at the top of the frame, before the shuffles and the fold search, so the one row per wave
// (coalesced, L2 resident) is in flight while those run.  An extension whose entry is -inf is dropped before the fold
// search; the others rank by v + (g + fmaf(alpha, entry, beta)), a stay candidate by its score + g.  A fold adds CTC mass
// only: g is a function of the token sequence, so the beam folded into holds the g the extension would have got.
#include "tmi_common.h"
#include <math.h>

namespace {

constexpr int CB_KMAX = 16;       // beams: one wave each
constexpr int CB_VMAX = 64;       // symbols: one lane each
constexpr int CB_TMAX = 65536;    // frames (trie node ids 1 + t K + r stay far inside int32)
constexpr int CB_PF = 4;          // frames per log-prob prefetch
constexpr uint32_t CB_MUL = 0x9E3779B1u;

struct CbBeam {
  float pb, pnb;
  int last, len, node, par;
  uint32_t hash;
  int pad;
};
struct CbBeamLm {
  float pb, pnb;
  int last, len, node, par;
  uint32_t hash;
  int ctx;  // the last order - 1 tokens, base V, the most recent one last; blank where the sequence has not begun
  float g;  // sum over the tokens of fmaf(alpha, lm entry, beta), in token order
  int pad;
};
template <bool LM> struct CbRec { using type = CbBeam; };
template <> struct CbRec<true> { using type = CbBeamLm; };

// What the fused form takes besides tmi_ctc_beam's arguments; the plain instantiation never reads it.
struct CbLmArgs {
  const float* lm;
  int ctx0, ctx_mod;  // the start context; V^(order-1)
  float alpha, beta;
  float *ctc_scores, *lm_scores;
};

__device__ __forceinline__ float cb_lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m));
}

// (score, candidate order) as one unsigned key; code = ext << 10 | k << 6 | c orders the candidates as K + k V + c does.
__device__ __forceinline__ uint64_t cb_key(float s, uint32_t code) {
  if (s == -INFINITY) return 0ull;
  if (s == 0.f) s = 0.f;  // (-0 and +0 are one score)
  uint32_t u = __float_as_uint(s);
  u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
  return ((uint64_t)u << 32) | (uint64_t)(0xFFFFFFFFu - code);
}

// Wave reductions of a 64-bit key without LDS traffic: DPP rotations inside each row of 16 lanes (row_ror 8, 4, 2, 1: every
// lane of a row ends with the row's maximum), then the four rows' values through scalar registers.
template <int CTRL> __device__ __forceinline__ uint64_t cb_dpp(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ uint64_t cb_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t cb_row_max(uint64_t v) {
  v = cb_max(v, cb_dpp<0x128>(v));
  v = cb_max(v, cb_dpp<0x124>(v));
  v = cb_max(v, cb_dpp<0x122>(v));
  return cb_max(v, cb_dpp<0x121>(v));
}
__device__ __forceinline__ uint64_t cb_lane(uint64_t v, int lane) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
}
__device__ __forceinline__ uint64_t cb_wave_max(uint64_t v) {
  v = cb_row_max(v);
  return cb_max(cb_max(cb_lane(v, 0), cb_lane(v, 16)), cb_max(cb_lane(v, 32), cb_lane(v, 48)));
}

// Is the sequence of trie node a the sequence of beam k (node b = (parent par_b, token last_b)), both of one length?  The
// record of b itself comes from the beam's registers: a node is stored at the end of the frame that created it, and only
// records of earlier frames are read here - their stores were complete at a barrier since.  Parents have smaller ids: the
// walk ends.
__device__ __forceinline__ bool cb_same(const int2* trie, int a, int b, int last_b, int par_b) {
  if (a == b) return true;
  if (a < 1 || b < 1) return false;
  const int2 first = trie[a - 1];
  if (first.y != last_b) return false;
  a = first.x;
  b = par_b;
  while (a != b) {
    if (a < 1 || b < 1) return false;
    const int2 ra = trie[a - 1], rb = trie[b - 1];
    if (ra.y != rb.y) return false;
    a = ra.x;
    b = rb.x;
  }
  return true;
}

template <bool LM>
__global__ __launch_bounds__(CB_KMAX* TMI_WAVE) void ctc_beam_kernel(const float* __restrict__ logp, int64_t lp_sn, int64_t lp_st,
                                                                    int V, const int32_t* __restrict__ frame_lens, int blank,
                                                                    int K, int32_t* __restrict__ tokens,
                                                                    int32_t* __restrict__ lengths, float* __restrict__ scores,
                                                                    int32_t* __restrict__ n_beams, int T_max, int2* trie_ws,
                                                                    CbLmArgs la) {
  using Rec = typename CbRec<LM>::type;
  __shared__ Rec s_beam[2][CB_KMAX];
  __shared__ float s_fold[CB_KMAX];
  __shared__ uint64_t s_head[2][CB_KMAX];
  const int n = blockIdx.x;
  int T = frame_lens[n];
  T = T > T_max ? T_max : T;  // (a value outside the contract never leads outside the tensors)
  const int k = threadIdx.x >> 6, c = threadIdx.x & 63;
  int2* trie = trie_ws + (int64_t)n * K * T_max;
  const bool sym = c < V;
  const float* __restrict__ lp = logp + (int64_t)n * lp_sn + (sym ? c : 0);

  // the start state: one empty beam
  float pb = 0.f, pnb = -INFINITY;
  int last = -1, len = 0, node = 0, par = 0, nb = 1;
  uint32_t hash = 0u;
  int ctx = 0;
  float g = 0.f;
  if constexpr (LM) {
    ctx = la.ctx0;
    if (threadIdx.x == 0) s_beam[0][0] = Rec{pb, pnb, last, len, node, par, hash, ctx, g, 0};
  } else {
    if (threadIdx.x == 0) s_beam[0][0] = Rec{pb, pnb, last, len, node, par, hash, 0};
  }
  if (threadIdx.x < CB_KMAX) s_fold[threadIdx.x] = -INFINITY;
  __syncthreads();

  float cur[CB_PF], nxt[CB_PF];
#pragma unroll
  for (int j = 0; j < CB_PF; ++j) cur[j] = (sym && j < T) ? lp[(int64_t)j * lp_st] : -INFINITY;
  for (int t0 = 0; t0 < T; t0 += CB_PF) {  // (every thread runs every frame: the barriers and shuffles are uniform)
#pragma unroll
    for (int j = 0; j < CB_PF; ++j) {
      const int t = t0 + CB_PF + j;
      nxt[j] = (sym && t < T) ? lp[(int64_t)t * lp_st] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < CB_PF; ++j) {
      const int t = t0 + j;
      if (t >= T) break;  // (uniform)
      const int rd = t & 1, wr = rd ^ 1;
      const bool live = k < nb;
      const bool ext = c != blank;
      float lmv = 0.f;
      if constexpr (LM) {
        if (live && sym && ext) lmv = la.lm[ctx * V + c];  // (ctx < V^(order-1): inside the table)
      }
      const float lpc = cur[j];
      const float lp_blank = __shfl(lpc, blank, 64);
      const float lp_e = __shfl(lpc, len > 0 ? last : 0, 64);
      const float tot = cb_lse2(pb, pnb);
      float n_pb = -INFINITY, n_pnb = -INFINITY, sc = -INFINITY;
      const uint32_t h_ext = hash * CB_MUL + (uint32_t)c + 1u;
      if (live && sym) {
        if (!ext) {
          n_pb = lp_blank + tot;
          n_pnb = len > 0 ? lp_e + pnb : -INFINITY;
        } else if (!LM || lmv != -INFINITY) {  // (a -inf entry: no candidate, nothing folded)
          const float v = lpc + ((len > 0 && c == last) ? pb : tot);
          int tgt = -1;
          for (int p = 0; p < nb; ++p) {
            const Rec& b = s_beam[rd][p];
            if (b.last == c && b.len == len + 1 && b.hash == h_ext && cb_same(trie, b.par, node, last, par)) {
              tgt = p;
              break;
            }
          }
          if (tgt >= 0) {
            s_fold[tgt] = v;  // (the beams of a set are distinct sequences: one extension at most folds into a beam)
          } else {
            n_pnb = v;
            sc = v;
          }
        }
      }
      __syncthreads();
      if (live && sym && !ext) {
        const float f = s_fold[k];
        if (f != -INFINITY) {
          n_pnb = cb_lse2(n_pnb, f);
          s_fold[k] = -INFINITY;
        }
        sc = cb_lse2(n_pb, n_pnb);
      }
      float g_c = g;
      if constexpr (LM) {
        if (ext) g_c = g + fmaf(la.alpha, lmv, la.beta);
        sc = sc == -INFINITY ? sc : sc + g_c;  // (the rank; the CTC score itself stays in n_pb, n_pnb)
      }
      uint64_t key = cb_key(sc, ((ext ? 1u : 0u) << 10) | ((uint32_t)k << 6) | (uint32_t)c);
      uint64_t best = cb_wave_max(key);
      if (c == 0) s_head[0][k] = best;
      __syncthreads();
      int nb_new = 0;
      for (int r = 0; r < K; ++r) {
        uint64_t w = c < K ? s_head[r & 1][c] : 0ull;
        w = cb_lane(cb_row_max(w), 0);  // (K <= 16: the heads sit in the first row of lanes)
        if (w == 0ull) break;  // (uniform over the workgroup: every wave read the same heads)
        const uint32_t code = 0xFFFFFFFFu - (uint32_t)w;
        if ((int)((code >> 6) & 15u) == k) {  // (uniform over the wave)
          if ((int)(code & 63u) == c) {
            if constexpr (LM) {
              s_beam[wr][r] = ext ? Rec{n_pb, n_pnb, c, len + 1, 1 + t * K + r, node, h_ext, (ctx * V + c) % la.ctx_mod, g_c, 0}
                                  : Rec{n_pb, n_pnb, last, len, node, par, hash, ctx, g, 0};
            } else {
              s_beam[wr][r] = ext ? Rec{n_pb, n_pnb, c, len + 1, 1 + t * K + r, node, h_ext, 0}
                                  : Rec{n_pb, n_pnb, last, len, node, par, hash, 0};
            }
            key = 0ull;
          }
          best = cb_wave_max(key);
        }
        if (c == 0) s_head[(r + 1) & 1][k] = best;
        nb_new = r + 1;
        __syncthreads();
      }
      nb = nb_new;
      if (k < nb) {
        const Rec& b = s_beam[wr][k];
        pb = b.pb, pnb = b.pnb, last = b.last, len = b.len, node = b.node, par = b.par, hash = b.hash;
        if constexpr (LM) ctx = b.ctx, g = b.g;
        if (c == 0 && node == 1 + t * K + k) trie[node - 1] = make_int2(par, last);  // created in this frame
      }
    }
#pragma unroll
    for (int j = 0; j < CB_PF; ++j) cur[j] = nxt[j];
  }

  __syncthreads();  // the last frame's trie nodes
  if (c == 0) {
    const int64_t o = (int64_t)n * K + k;
    if (k < nb) {
      lengths[o] = len;
      const float ctc = cb_lse2(pb, pnb);
      if constexpr (LM) {
        scores[o] = ctc + g;
        la.ctc_scores[o] = ctc;
        la.lm_scores[o] = g;
      } else {
        scores[o] = ctc;
      }
      int32_t* row = tokens + o * T_max;
      int a = node;
      for (int pos = len - 1; pos >= 0 && a >= 1; --pos) {
        const int2 rec = trie[a - 1];
        row[pos] = rec.y;
        a = rec.x;
      }
    } else {
      lengths[o] = 0;
      scores[o] = -INFINITY;
      if constexpr (LM) {
        la.ctc_scores[o] = -INFINITY;
        la.lm_scores[o] = 0.f;
      }
    }
    if (k == 0) n_beams[n] = nb;
  }
}

}  // namespace

extern "C" int64_t tmi_ctc_beam_workspace_bytes(int64_t N, int64_t K, int64_t T_max) {
  if (N < 1 || N > 65535 || K < 1 || K > CB_KMAX || T_max < 1 || T_max > CB_TMAX) return -1;
  return N * K * T_max * (int64_t)sizeof(int2);
}

static bool cb_bad_args(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* frame_lens, int32_t blank,
                        int32_t K, int32_t* tokens, int32_t* lengths, float* scores, int32_t* n_beams, int64_t N, int64_t T_max,
                        void* workspace, int64_t workspace_bytes) {
  const int64_t need = tmi_ctc_beam_workspace_bytes(N, K, T_max);
  return !logp || !frame_lens || !tokens || !lengths || !scores || !n_beams || !workspace || !tmi_aligned(logp, 4) ||
         !tmi_aligned(frame_lens, 4) || !tmi_aligned(tokens, 4) || !tmi_aligned(lengths, 4) || !tmi_aligned(scores, 4) ||
         !tmi_aligned(n_beams, 4) || !tmi_aligned(workspace, 8) || need < 0 || workspace_bytes < need || V < 2 || V > CB_VMAX ||
         lp_st < V || lp_st > ((int64_t)1 << 30) || lp_sn < T_max * lp_st || blank < 0 || blank >= V;
}

static int tmi_ctc_beam_impl(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* frame_lens,
                             int32_t blank, int32_t K, int32_t* tokens, int32_t* lengths, float* scores, int32_t* n_beams,
                             int64_t N, int64_t T_max, void* workspace, int64_t workspace_bytes, void* stream) {
  if (cb_bad_args(logp, lp_sn, lp_st, V, frame_lens, blank, K, tokens, lengths, scores, n_beams, N, T_max, workspace,
                  workspace_bytes)) {
    tmi_set_error("tmi_ctc_beam: bad argument (non-NULL 4-byte aligned pointers, the workspace 8-byte aligned; 1 <= N <= 65535 "
                  "items, one workgroup each; 1 <= K <= 16 beams, one wave each; 2 <= V <= 64 symbols, one lane each; "
                  "1 <= T_max <= 65536 frames; V <= lp_st <= 2^30, lp_sn >= T_max lp_st; 0 <= blank < V; workspace of "
                  "tmi_ctc_beam_workspace_bytes)");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(ctc_beam_kernel<false>, dim3((unsigned)N), dim3((unsigned)K * TMI_WAVE), 0,
                     reinterpret_cast<hipStream_t>(stream), logp, lp_sn, lp_st, (int)V, frame_lens, (int)blank, (int)K, tokens,
                     lengths, scores, n_beams, (int)T_max, reinterpret_cast<int2*>(workspace), CbLmArgs{});
  return tmi_check_launch("tmi_ctc_beam");
}

extern "C" int tmi_ctc_beam(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* frame_lens, int32_t blank,
                            int32_t K, int32_t* tokens, int32_t* lengths, float* scores, int32_t* n_beams, int64_t N,
                            int64_t T_max, void* workspace, int64_t workspace_bytes, void* stream) {
  return tmi_plan_run<tmi_ctc_beam_impl>(logp, lp_sn, lp_st, V, frame_lens, blank, K, tokens, lengths, scores, n_beams, N, T_max,
                                         workspace, workspace_bytes, stream);
}

static int tmi_ctc_beam_lm_impl(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* frame_lens,
                                int32_t blank, int32_t K, const float* lm, int32_t lm_order, float lm_alpha, float lm_beta,
                                int32_t* tokens, int32_t* lengths, float* scores, float* ctc_scores, float* lm_scores,
                                int32_t* n_beams, int64_t N, int64_t T_max, void* workspace, int64_t workspace_bytes,
                                void* stream) {
  bool bad = cb_bad_args(logp, lp_sn, lp_st, V, frame_lens, blank, K, tokens, lengths, scores, n_beams, N, T_max, workspace,
                         workspace_bytes) ||
             !lm || !ctc_scores || !lm_scores || !tmi_aligned(lm, 4) || !tmi_aligned(ctc_scores, 4) ||
             !tmi_aligned(lm_scores, 4) || lm_order < 1 || lm_order > 4 || !isfinite(lm_alpha) || lm_alpha < 0.f ||
             !isfinite(lm_beta);
  int64_t ctx_mod = 1, ctx0 = 0;  // V^(order-1); blank (1 + V + ... + V^(order-2))
  if (!bad) {
    for (int i = 1; i < lm_order; ++i) {
      ctx0 = ctx0 * V + blank;
      ctx_mod *= V;
    }
    bad = ctx_mod * V > ((int64_t)1 << 24);
  }
  if (bad) {
    tmi_set_error("tmi_ctc_beam_lm: bad argument (tmi_ctc_beam's limits; lm, ctc_scores and lm_scores non-NULL and 4-byte "
                  "aligned; 1 <= lm_order <= 4 with V^lm_order <= 2^24 table entries; lm_alpha >= 0 and lm_beta finite)");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(ctc_beam_kernel<true>, dim3((unsigned)N), dim3((unsigned)K * TMI_WAVE), 0,
                     reinterpret_cast<hipStream_t>(stream), logp, lp_sn, lp_st, (int)V, frame_lens, (int)blank, (int)K, tokens,
                     lengths, scores, n_beams, (int)T_max, reinterpret_cast<int2*>(workspace),
                     CbLmArgs{lm, (int)ctx0, (int)ctx_mod, lm_alpha, lm_beta, ctc_scores, lm_scores});
  return tmi_check_launch("tmi_ctc_beam_lm");
}

extern "C" int tmi_ctc_beam_lm(const float* logp, int64_t lp_sn, int64_t lp_st, int64_t V, const int32_t* frame_lens,
                               int32_t blank, int32_t K, const float* lm, int32_t lm_order, float lm_alpha, float lm_beta,
                               int32_t* tokens, int32_t* lengths, float* scores, float* ctc_scores, float* lm_scores,
                               int32_t* n_beams, int64_t N, int64_t T_max, void* workspace, int64_t workspace_bytes,
                               void* stream) {
  return tmi_plan_run<tmi_ctc_beam_lm_impl>(logp, lp_sn, lp_st, V, frame_lens, blank, K, lm, lm_order, lm_alpha, lm_beta, tokens,
                                            lengths, scores, ctc_scores, lm_scores, n_beams, N, T_max, workspace,
                                            workspace_bytes, stream);
}
