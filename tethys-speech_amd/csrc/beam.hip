// Beam search's per-step bookkeeping: tmi_beam_step (the decoding rule of whisper.py's generate, written out there and in
// include/tethys_mi.h).
//
// One workgroup per batch item; everything it touches is the item's own: K running sums, K prefix rows, the K-entry
// pool of finished hypotheses, the done flag.  The K * N candidates are staged in LDS and ranked by counting (score
// desc, then (beam, column) asc: every candidate's rank is distinct, no sort), the walk over the 2K best ranks is one
// thread's (at most 16 ranks and 8 pool entries), and the rows move with the whole workgroup.  The pool is kept sorted in
// place: an entry only ever moves to a higher slot (an insertion pushes the ones behind it down, an eviction drops the
// last), so its rows are moved slot by slot from the back, each thread always on the same columns - no barrier needed
// between the moves.  All fp32 arithmetic is one IEEE add per candidate and one correctly rounded division per
// normalised score, so a host restatement in fp32 matches it bit for bit.
#include "tmi_common.h"

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_KMAX = 8;

__global__ __launch_bounds__(BS_THREADS) void beam_step_kernel(
    const int32_t* __restrict__ cand_ids, const float* __restrict__ cand_lp, int N, int K, float* __restrict__ sums,
    const int32_t* __restrict__ cur, int32_t* __restrict__ nxt, int64_t ld, int t, int eos_id, float len_pow,
    int early_stopping, int32_t* __restrict__ pool_ids, float* __restrict__ pool_scores, int32_t* __restrict__ pool_len,
    int32_t* __restrict__ pool_cnt, int32_t* __restrict__ done, int32_t* __restrict__ done_count, int finalize) {
  __shared__ float c_sc[BS_KMAX * 16];
  __shared__ int c_v[BS_KMAX * 16];
  __shared__ float s_sum[BS_KMAX];
  __shared__ float sel_sc[2 * BS_KMAX];
  __shared__ int sel_k[2 * BS_KMAX], sel_v[2 * BS_KMAX];
  __shared__ float ps[BS_KMAX];                      // pool scores, sorted
  __shared__ int pl[BS_KMAX], psrc[BS_KMAX];         // lengths; source: old slot q >= 0, or new hypothesis -(1 + h)
  __shared__ int h_par[BS_KMAX], h_tok[BS_KMAX];     // new hypotheses: parent beam, last token
  __shared__ int nb_k[BS_KMAX], nb_v[BS_KMAX];       // the next live beams: parent, token
  __shared__ float nb_s[BS_KMAX];
  __shared__ int s_done, s_cnt, s_live;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t rb = (int64_t)b * K;
  if (tid == 0) s_done = done[b];
  if (tid < K) s_sum[tid] = sums[rb + tid];
  __syncthreads();
  if (s_done) {  // frozen: the next prefix rows stay valid, nothing else moves
    if (!finalize)
      for (int64_t i = tid; i < (int64_t)K * t; i += BS_THREADS) {
        const int64_t k = i / t, c = i % t;
        nxt[(rb + k) * ld + c] = cur[(rb + k) * ld + c];
      }
    return;
  }

  if (!finalize) {
    const int KN = K * N;
    if (tid < KN) {
      const int k = tid / N;
      c_sc[tid] = s_sum[k] + cand_lp[rb * N + tid];
      c_v[tid] = cand_ids[rb * N + tid];
    }
    __syncthreads();
    if (tid < KN) {
      const float sc = c_sc[tid];
      const int k = tid / N, v = c_v[tid];
      int rank = 0;
      for (int i = 0; i < KN; ++i) {
        const float o = c_sc[i];
        const int ok = i / N, ov = c_v[i];
        rank += o > sc || (o == sc && (ok < k || (ok == k && ov < v)));
      }
      if (rank < 2 * K) {
        sel_sc[rank] = sc;
        sel_k[rank] = k;
        sel_v[rank] = v;
      }
    }
    __syncthreads();
  }

  // ---- the walk (one thread): offers to the pool, the next live beams, the stop test
  if (tid == 0) {
    int cnt = pool_cnt[b];
    for (int p = 0; p < cnt; ++p) {
      ps[p] = pool_scores[rb + p];
      pl[p] = pool_len[rb + p];
      psrc[p] = p;
    }
    int nh = 0;
    auto offer = [&](float score, int parent, int tok) {
      int pos;
      if (cnt < K) {
        pos = cnt++;
      } else if (score > ps[K - 1]) {
        pos = K - 1;
      } else {
        return;
      }
      for (; pos > 0 && ps[pos - 1] < score; --pos) {
        ps[pos] = ps[pos - 1];
        pl[pos] = pl[pos - 1];
        psrc[pos] = psrc[pos - 1];
      }
      ps[pos] = score;
      pl[pos] = t;
      psrc[pos] = -(1 + nh);
      h_par[nh] = parent;
      h_tok[nh] = tok;
      ++nh;
    };
    int live = 0;
    if (!finalize) {
      for (int j = 0; j < 2 * K; ++j) {
        const int v = sel_v[j], k = sel_k[j];
        if (eos_id >= 0 && v == eos_id) {
          if (j < K) offer(__fdiv_rn(sel_sc[j], len_pow), k, v);
          continue;
        }
        if (live < K) {
          nb_k[live] = k;
          nb_v[live] = v;
          nb_s[live] = sel_sc[j];
          ++live;
        }
      }
      if (cnt == K && live > 0 && (early_stopping || ps[K - 1] >= __fdiv_rn(nb_s[0], len_pow))) {
        done[b] = 1;
        atomicAdd(done_count, 1);
      }
    } else {
      for (int k = 0; k < K; ++k) offer(__fdiv_rn(s_sum[k], len_pow), k, cur[(rb + k) * ld + t]);
    }
    for (int p = 0; p < cnt; ++p) {
      pool_scores[rb + p] = ps[p];
      pool_len[rb + p] = pl[p];
    }
    pool_cnt[b] = cnt;
    s_cnt = cnt;
    s_live = live;
  }
  __syncthreads();

  // ---- the pool's rows, from the back (an entry's source slot is never above its new slot)
  int32_t* prow = pool_ids + rb * ld;
  for (int p = s_cnt - 1; p >= 0; --p) {
    const int src = psrc[p];
    if (src == p) continue;
    if (src >= 0) {
      for (int c = tid; c <= pl[p]; c += BS_THREADS) prow[p * ld + c] = prow[src * ld + c];
    } else {
      const int h = -1 - src;
      const int32_t* par = cur + (rb + h_par[h]) * ld;
      for (int c = tid; c <= t; c += BS_THREADS) prow[p * ld + c] = c < t ? par[c] : h_tok[h];
    }
  }
  if (finalize) return;

  // ---- the next live beams
  for (int64_t i = tid; i < (int64_t)s_live * (t + 1); i += BS_THREADS) {
    const int n = (int)(i / (t + 1)), c = (int)(i % (t + 1));
    nxt[(rb + n) * ld + c] = c < t ? cur[(rb + nb_k[n]) * ld + c] : nb_v[n];
  }
  if (tid < s_live) sums[rb + tid] = nb_s[tid];
}

}  // namespace

static int tmi_beam_step_impl(const int32_t* cand_ids, const float* cand_lp, int64_t N, int64_t B, int64_t K, float* sums,
                              const int32_t* cur, int32_t* nxt, int64_t ld, int64_t t, int32_t eos_id, float len_pow,
                              int32_t early_stopping, int32_t* pool_ids, float* pool_scores, int32_t* pool_len,
                              int32_t* pool_cnt, int32_t* done, int32_t* done_count, int32_t finalize, void* stream) {
  const bool step_ok = finalize ? true : (cand_ids && cand_lp && nxt && N >= 2 * K && N <= 16);
  if (!step_ok || !sums || !cur || !pool_ids || !pool_scores || !pool_len || !pool_cnt || !done || !done_count ||
      B < 1 || B > 65535 || K < 1 || K > BS_KMAX || t < 1 || t >= ld || ld > INT32_MAX ||
      !(len_pow > 0.f && len_pow < INFINITY) || (finalize != 0 && finalize != 1)) {
    tmi_set_error("tmi_beam_step: bad argument");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)B), dim3(BS_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     cand_ids, cand_lp, (int)N, (int)K, sums, cur, nxt, ld, (int)t, eos_id, len_pow, early_stopping,
                     pool_ids, pool_scores, pool_len, pool_cnt, done, done_count, finalize);
  return tmi_check_launch("tmi_beam_step");
}
extern "C" int tmi_beam_step(const int32_t* cand_ids, const float* cand_lp, int64_t N, int64_t B, int64_t K, float* sums,
                             const int32_t* cur, int32_t* nxt, int64_t ld, int64_t t, int32_t eos_id, float len_pow,
                             int32_t early_stopping, int32_t* pool_ids, float* pool_scores, int32_t* pool_len,
                             int32_t* pool_cnt, int32_t* done, int32_t* done_count, int32_t finalize, void* stream) {
  return tmi_plan_run<tmi_beam_step_impl>(cand_ids, cand_lp, N, B, K, sums, cur, nxt, ld, t, eos_id, len_pow, early_stopping,
                                          pool_ids, pool_scores, pool_len, pool_cnt, done, done_count, finalize, stream);
}
