// Scoring kernels of the evaluation paths.  First, teacher-forced scoring: tmi_logprob_fold (W:585-600 without the gradient,
// SparseCategoricalAccuracy of W:904-907).  Behind it, with a header comment of their own, the Wav2Vec2 evaluation kernels
// tmi_contrastive_score and tmi_vq_count.
//
// The LM head of an evaluation pass is computed by tmi_gemm in column chunks of tmi_logprob_chunk_cols() columns into a
// scratch [M, chunk] buffer; after each chunk this kernel folds it into 32 bytes of running state per row - the online
// softmax pair (max, sum exp(z - max)), the best argmax key and the target logit - so that the [M, 51904] logits never
// exist.  The chunk was written a moment ago by the GEMM and is read once, from the Infinity Cache when it fits.
//
// Form (cdna_hip_programming.md, memory-bound recipe): one wave per row, four rows per 256-thread workgroup, 16-byte
// loads of the row (8 bf16 / 4 fp32 columns per lane and trip), max / exp / sum in fp32.  Every order is fixed: a lane
// folds its own vectors in column order, the 64 lane partials meet in a butterfly that pairs the lower lane first (the
// lse fold of decode.hip), and the chunk's result joins the running state behind the earlier chunks.  With a fixed chunk
// width the outputs are therefore bit-reproducible; there are no atomics and the state has no zero-before-use contract
// (first = 1 overwrites it).
//
// Argmax: decode.hip's 64-bit key, order-preserving float bits << 32 | ~column with -0 folded onto +0: the largest stored
// logit wins, the smallest column among equals.  The column is the global one, so "a later chunk replaces the running best
// only when strictly greater" is the plain comparison of keys.
//
// Target logit: fp32 chunks carry it; for bf16 chunks the row's wave recomputes x[r, :] . w[:, target] in fp32 from the
// GEMM's operands (the note on tmi_linear_xent in include/tethys_mi.h), in the chunk that holds the target's column.
#include "tmi_common.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_ROWS = LP_THREADS / TMI_WAVE;  // rows per workgroup
constexpr int64_t LP_CHUNK_COLS = 8192;         // tmi_logprob_chunk_cols(): a multiple of the fast GEMM's widest N tile (256)

struct LpState {  // tmi_logprob_state_bytes(M) = 32 * M
  float m, s;     // max and sum exp(z - m) over the real columns seen so far
  uint64_t best;  // argmax key (0: none yet)
  float zt;       // the target logit, once its chunk has been folded
  float zts;      // the target logit as the chunk stores it (== zt unless zt was recomputed)
  float pad[2];
};
static_assert(sizeof(LpState) == 32, "state layout");

template <typename T> struct lp_vec;
template <> struct lp_vec<bf16_t> {
  static constexpr int N = 8;
  u32x4 r;
  __device__ __forceinline__ void load(const bf16_t* p) { r = *reinterpret_cast<const u32x4*>(p); }
  __device__ __forceinline__ float get(int c) const {
    const uint32_t w = r[c >> 1];
    return __uint_as_float((c & 1) ? (w & 0xffff0000u) : (w << 16));
  }
};
template <> struct lp_vec<float> {
  static constexpr int N = 4;
  u32x4 r;
  __device__ __forceinline__ void load(const float* p) { r = *reinterpret_cast<const u32x4*>(p); }
  __device__ __forceinline__ float get(int c) const { return __uint_as_float(r[c]); }
};

template <typename T>
__global__ __launch_bounds__(LP_THREADS) void lp_fold_kernel(
    const T* __restrict__ chunk, int64_t ld, int M, int V, int col0, int nreal, const int32_t* __restrict__ targets,
    const bf16_t* __restrict__ x, int64_t x_ld, const bf16_t* __restrict__ w, int64_t w_sk, int64_t w_sn, int d,
    LpState* __restrict__ state, int first, int last, float* __restrict__ lse, float* __restrict__ logprob,
    int32_t* __restrict__ argmax) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * LP_ROWS + (threadIdx.x >> 6);
  if (row >= M) return;  // (whole waves: no barrier follows)
  constexpr int N = lp_vec<T>::N;
  const T* __restrict__ p = chunk + (int64_t)row * ld;

  // ---- this lane's columns j, j + 64 N, ...: online softmax and best key over the real columns [0, nreal) of the chunk
  float am = -INFINITY, as = 0.f;
  uint64_t best = 0;
  for (int j = lane * N; j < nreal; j += 64 * N) {  // (ld is a multiple of N and nreal <= ld: the 16 bytes are inside the row)
    lp_vec<T> v;
    v.load(p + j);
    float z[N];
    float vm = -INFINITY;
#pragma unroll
    for (int c = 0; c < N; ++c) {
      const bool ok = j + c < nreal;  // a pad column is loaded with its vector and never looked at
      z[c] = ok ? v.get(c) : -INFINITY;
      if (ok) {
        vm = fmaxf(vm, z[c]);
        const uint64_t key = ((uint64_t)am_order(z[c]) << 32) | (uint64_t)(~(uint32_t)(col0 + j + c));
        if (key > best) best = key;
      }
    }
    if (vm > am) {  // (vm == -inf: nothing to add; am == -inf: as is 0 and exp(-inf) = 0)
      as *= __expf(am - vm);
      am = vm;
    }
    if (am != -INFINITY) {
      float vs = 0.f;
#pragma unroll
      for (int c = 0; c < N; ++c) vs += __expf(z[c] - am);  // (exp(-inf) = 0 for the columns left out)
      as += vs;
    }
  }

  // ---- the 64 partials: a butterfly that pairs the lower lane first, in both lanes
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float om = __shfl_xor(am, o, 64), os = __shfl_xor(as, o, 64);
    if (lane & o) {
      float lm = om, ls = os;
      lse_fold(lm, ls, am, as);
      am = lm, as = ls;
    } else {
      lse_fold(am, as, om, os);
    }
    const uint32_t lo = __shfl_xor((uint32_t)best, o, 64), hi = __shfl_xor((uint32_t)(best >> 32), o, 64);
    const uint64_t ob = ((uint64_t)hi << 32) | lo;
    if (ob > best) best = ob;
  }

  // ---- the target logit, in the chunk that holds its column (a target outside [0, V) is in no chunk)
  const int t = targets[row];
  const bool here = t >= col0 && t < col0 + nreal;
  float zt = 0.f, zts = 0.f;
  if (here) {  // (uniform over the wave)
    zt = zts = to_f32(p[t - col0]);
    if (x != nullptr) {
      float acc = 0.f;
      for (int k = lane; k < d; k += 64)
        acc = fmaf((float)x[(int64_t)row * x_ld + k], (float)w[(int64_t)k * w_sk + (int64_t)t * w_sn], acc);
      zt = wave_sum(acc);
    }
  }

  if (lane != 0) return;
  LpState st;
  if (first) {
    st.m = am, st.s = as, st.best = best, st.zt = zt, st.zts = zts;
  } else {
    st = state[row];
    lse_fold(st.m, st.s, am, as);        // the earlier chunks first
    if (best > st.best) st.best = best;  // (keys of different columns are never equal: strictly greater value, or an equal one at a smaller column - which an earlier chunk holds)
    if (here) st.zt = zt, st.zts = zts;
  }
  st.pad[0] = st.pad[1] = 0.f;
  if (!last) {
    state[row] = st;
    return;
  }
  const float l = st.m + logf(st.s);
  lse[row] = l;
  float lp;
  if (t == -1) {
    lp = 0.f;
  } else if (t < 0 || t >= V) {
    lp = __uint_as_float(0x7fc00000u);  // never found in any chunk: flagged with NaN instead of a number that looks like a score
  } else if (x != nullptr) {
    // tmi_linear_xent's form (softmax_xent.hip): both terms of the loss see the SAME target logit - the target's term of the
    // sum is swapped for exp(zt) too, or a row whose target dominates keeps the rounding error of the stored logit and can
    // come out positive.  log1p(sum of the OTHER terms * exp(m - zt)): non-negative, free of the m + log(s) - zt cancellation.
    const float rest = fmaxf(st.s - expf(st.zts - st.m), 0.f);
    const float dz = st.m - st.zt;
    lp = -(dz < 80.f ? log1pf(rest * expf(dz)) : dz + logf(rest));
  } else {
    lp = st.zt - l;
  }
  logprob[row] = lp;
  argmax[row] = (int32_t)(~(uint32_t)st.best);
}

}  // namespace

extern "C" int64_t tmi_logprob_state_bytes(int64_t M) { return M < 1 ? -1 : (int64_t)sizeof(LpState) * M; }
extern "C" int64_t tmi_logprob_chunk_cols(void) { return LP_CHUNK_COLS; }

static int tmi_logprob_fold_impl(const void* chunk, int64_t ld, int32_t dtype, int64_t M, int64_t V, int64_t col0, int64_t ncols,
                                 const int32_t* targets, const void* x, int64_t x_ld, const void* w, int64_t w_sk,
                                 int64_t w_sn, int64_t d, void* state, int64_t state_bytes, int32_t first, int32_t last,
                                 float* lse, float* logprob, int32_t* argmax, void* stream) {
  const bool dt_ok = dtype == TMI_F32 || dtype == TMI_BF16;
  const int64_t vec = dtype == TMI_BF16 ? 8 : 4;
  const bool lm = x != nullptr || w != nullptr;
  const bool lm_ok = !lm || (x && w && d >= 1 && d <= (1 << 20) && x_ld >= d && w_sk != 0 && w_sn != 0 && tmi_aligned(x, 2) && tmi_aligned(w, 2));
  const bool out_ok = !last || (lse && logprob && argmax && tmi_aligned(lse, 4) && tmi_aligned(logprob, 4) && tmi_aligned(argmax, 4));
  if (!chunk || !targets || !tmi_aligned(targets, 4) || !state || !dt_ok || !lm_ok || !out_ok || M < 1 || M > (1 << 30) || V < 1 || V > (1 << 30) ||
      col0 < 0 || col0 >= V || ncols < 1 || ncols > ld || ld > (1 << 30) || (ld % vec) != 0 || !tmi_aligned(chunk, 16) ||
      !tmi_aligned(state, 8) || state_bytes < (int64_t)sizeof(LpState) * M || (first != 0 && first != 1) || (last != 0 && last != 1) ||
      (first && col0 != 0) || (!first && col0 == 0) || (last && col0 + ncols < V) || (!last && col0 + ncols >= V)) {
    tmi_set_error("tmi_logprob_fold: bad argument");
    return TMI_ERR_INVALID;
  }
  const int64_t nreal = V - col0 < ncols ? V - col0 : ncols;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((M + LP_ROWS - 1) / LP_ROWS));
  LpState* st = reinterpret_cast<LpState*>(state);
  if (dtype == TMI_BF16)
    // (the fp32 recomputation applies to bf16 chunks with operands given)
    hipLaunchKernelGGL(lp_fold_kernel<bf16_t>, grid, dim3(LP_THREADS), 0, s, reinterpret_cast<const bf16_t*>(chunk), ld, (int)M,
                       (int)V, (int)col0, (int)nreal, targets, reinterpret_cast<const bf16_t*>(x), x_ld,
                       reinterpret_cast<const bf16_t*>(w), w_sk, w_sn, (int)d, st, first, last, lse, logprob, argmax);
  else
    hipLaunchKernelGGL(lp_fold_kernel<float>, grid, dim3(LP_THREADS), 0, s, reinterpret_cast<const float*>(chunk), ld, (int)M,
                       (int)V, (int)col0, (int)nreal, targets, (const bf16_t*)nullptr, (int64_t)0, (const bf16_t*)nullptr,
                       (int64_t)0, (int64_t)0, 0, st, first, last, lse, logprob, argmax);
  return tmi_check_launch("tmi_logprob_fold");
}

extern "C" int tmi_logprob_fold(const void* chunk, int64_t ld, int32_t dtype, int64_t M, int64_t V, int64_t col0, int64_t ncols,
                                const int32_t* targets, const void* x, int64_t x_ld, const void* w, int64_t w_sk, int64_t w_sn,
                                int64_t d, void* state, int64_t state_bytes, int32_t first, int32_t last, float* lse,
                                float* logprob, int32_t* argmax, void* stream) {
  return tmi_plan_run<tmi_logprob_fold_impl>(chunk, ld, dtype, M, V, col0, ncols, targets, x, x_ld, w, w_sk, w_sn, d, state,
                                             state_bytes, first, last, lse, logprob, argmax, stream);
}

// ---------------------------------------------------------------- Wav2Vec2 evaluation: tmi_contrastive_score, tmi_vq_count
// The contrastive loss of V:866-899 in gathered form, forward only: row (b, t) takes the dot products of h_t with q_t and
// with the q rows its negative indices name - O(T N d) - instead of reading them out of the all-pairs [T, T] product that
// tmi_contrastive_fwd_bwd needs for its gradient.  Frames whose mask is not > 0 score nothing as a query (loss 0, correct 0)
// and are dropped from every softmax as a negative; so is an index outside [0, T), which is never dereferenced.
//
// Form: one wave per row, four rows per 256-thread workgroup.  The wave stages h_t once in LDS in its stored type (CS_KC
// elements at a time; the projection widths of every model fit one piece); item 0 is the positive (frame t), item n >= 1
// the n-th negative; lane l owns the items l, l + 64, ... and reads "its" q row with 16-byte loads (8 bf16 / 4 fp32), q
// staying in L2 (400 KB at the workload's size).
// Arithmetic order, the same for every item - a negative equal to t therefore reproduces the positive's logit bit for bit:
//   dot   = fma chain over k = 0 .. pd-1 in ascending k from 0.f (fp32, operands as stored: pd roundings)
//   logit = dot * (1.f / temperature)                        (the reciprocal is taken once on the host: 2 roundings)
// A lane folds its items in ascending order into an online pair (m, s = sum exp(z - m)); the row maximum is the exact
// wave_max of the lane maxima, each lane rescales its own sum once, s * expf(m - max) (a lane with one item: 1 * expf(z - max)),
// and the 64 sums meet in the xor butterfly of wave_sum (lane distance 32, 16, .., 1): fixed order, no atomics, no
// workspace, bit-reproducible.  loss = (max - logit_0) + logf(sum), tmi_contrastive_fwd_bwd's form: it never rounds at the
// size of the logits and is >= 0 (the lane holding the maximum contributes s >= 1).  correct = logit_0 >= every kept
// negative logit (tf.argmax: the first index wins a tie).
constexpr int CS_THREADS = 256;
constexpr int CS_ROWS = CS_THREADS / TMI_WAVE;
constexpr int CS_KC = 1024;  // elements of h_t staged at a time

namespace {

template <typename T>
__global__ __launch_bounds__(CS_THREADS) void cs_kernel(const T* __restrict__ h, const T* __restrict__ q, int64_t ld,
                                                        const int32_t* __restrict__ neg, int64_t neg_sb, int64_t neg_st,
                                                        const float* __restrict__ mask, int64_t rows, int Tn, int pd, int Nn,
                                                        float inv_temp, float* __restrict__ row_loss,
                                                        int32_t* __restrict__ row_correct) {
  __shared__ __attribute__((aligned(16))) T hs[CS_ROWS][CS_KC];
  constexpr int N = lp_vec<T>::N;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * CS_ROWS + w;
  const bool live = row < rows;
  const int64_t r = live ? row : rows - 1;  // (a wave past the end walks the last row and stores nothing: the barriers below are block-wide)
  const int64_t b = r / Tn;
  const int t = (int)(r % Tn);
  const float* __restrict__ mb = mask ? mask + b * Tn : nullptr;
  const bool valid = live && (!mb || mb[t] > 0.f);
  const T* __restrict__ hr = h + r * ld;
  const T* __restrict__ qb = q + b * Tn * ld;
  const int32_t* __restrict__ nb = neg + b * neg_sb + (int64_t)t * neg_st;

  float m = -INFINITY, s = 0.f, l0 = 0.f, mneg = -INFINITY;
  for (int i0 = 0; i0 <= Nn; i0 += 64) {  // (Nn and pd are uniform over the workgroup: so is every barrier)
    const int it = i0 + lane;
    int j = -1;  // the frame this lane scores against, -1: none
    if (valid && it <= Nn) {
      j = it == 0 ? t : nb[it - 1];
      if (j < 0 || j >= Tn || (it > 0 && mb && !(mb[j] > 0.f))) j = -1;
    }
    float acc = 0.f;
    for (int k0 = 0; k0 < pd; k0 += CS_KC) {
      const int kc = pd - k0 < CS_KC ? pd - k0 : CS_KC;
      if (pd > CS_KC || i0 == 0) {
        __syncthreads();
        for (int k = lane * N; k < kc; k += 64 * N)
          *reinterpret_cast<u32x4*>(&hs[w][k]) = *reinterpret_cast<const u32x4*>(hr + k0 + k);
        __syncthreads();
      }
      if (j >= 0) {
        const T* __restrict__ qr = qb + (int64_t)j * ld + k0;
        for (int k = 0; k < kc; k += N) {
          lp_vec<T> a, c;
          a.load(&hs[w][k]);
          c.load(qr + k);
#pragma unroll
          for (int e = 0; e < N; ++e) acc = fmaf(a.get(e), c.get(e), acc);
        }
      }
    }
    if (j >= 0) {
      const float z = acc * inv_temp;
      if (it == 0) l0 = z; else mneg = fmaxf(mneg, z);
      if (z > m) {  // (m == -inf: s is 0 and expf(-inf) = 0)
        s = s * expf(m - z) + 1.f;
        m = z;
      } else {
        s += expf(z - m);
      }
    }
  }
  const float mx = wave_max(m);
  const float sum = wave_sum(m == -INFINITY ? 0.f : s * expf(m - mx));
  l0 = __shfl(l0, 0, 64);
  mneg = wave_max(mneg);
  if (lane != 0 || !live) return;
  row_loss[row] = valid ? (mx - l0) + logf(sum) : 0.f;  // (no kept negative: max == logit_0 and sum == 1, so exactly 0)
  row_correct[row] = valid && l0 >= mneg ? 1 : 0;
}

// counts[g][clamp(idx[r][g])] += 1 over the valid rows: an LDS histogram per workgroup, then one 64-bit atomic add per
// non-empty bin.  Integer adds only: exact, whatever the order.
__global__ __launch_bounds__(256) void vq_count_kernel(const int32_t* __restrict__ idx, const float* __restrict__ mask,
                                                       unsigned long long* __restrict__ counts, int64_t rows, int G, int Nc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* cnt = reinterpret_cast<uint32_t*>(smem);  // [G * Nc]
  const int bins = G * Nc;
  for (int i = threadIdx.x; i < bins; i += 256) cnt[i] = 0u;
  __syncthreads();
  const int64_t total = rows * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    if (mask && !(mask[i / G] > 0.f)) continue;
    int bi = idx[i];
    bi = bi < 0 ? 0 : (bi >= Nc ? Nc - 1 : bi);  // as vq_assign_kernel: the code counted is the code assigned
    atomicAdd(&cnt[(int)(i % G) * Nc + bi], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += 256)
    if (cnt[i]) atomicAdd(&counts[i], (unsigned long long)cnt[i]);
}

}  // namespace

static int tmi_contrastive_score_impl(const void* h, const void* q, int64_t ld, int32_t dtype, const int32_t* neg, int64_t neg_sb,
                                      int64_t neg_st, const float* mask, float* row_loss, int32_t* row_correct, int64_t B,
                                      int64_t T, int64_t pd, int64_t Nn, float temperature, void* stream) {
  const bool dt_ok = dtype == TMI_F32 || dtype == TMI_BF16;
  const int64_t vec = dtype == TMI_BF16 ? 8 : 4;
  const int64_t lim = (int64_t)1 << 30;
  if (!h || !q || !neg || !row_loss || !row_correct || !dt_ok || !tmi_aligned(h, 16) || !tmi_aligned(q, 16) || !tmi_aligned(neg, 4) ||
      !tmi_aligned(mask, 4) || !tmi_aligned(row_loss, 4) || !tmi_aligned(row_correct, 4) || B < 1 || T < 1 || Nn < 1 || pd < 1 || B > lim ||
      T > lim || Nn > lim || pd > lim || ld > lim || B * T > lim || (pd % vec) != 0 || ld < pd || (ld % vec) != 0 ||
      neg_sb < 0 || neg_st < 0 || !(temperature > 0.f)) {
    tmi_set_error("tmi_contrastive_score: bad argument");
    return TMI_ERR_INVALID;
  }
  const int64_t rows = B * T;
  const dim3 grid((unsigned)((rows + CS_ROWS - 1) / CS_ROWS));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const float inv_temp = 1.0f / temperature;
  if (dtype == TMI_BF16)
    hipLaunchKernelGGL(cs_kernel<bf16_t>, grid, dim3(CS_THREADS), 0, s, reinterpret_cast<const bf16_t*>(h),
                       reinterpret_cast<const bf16_t*>(q), ld, neg, neg_sb, neg_st, mask, rows, (int)T, (int)pd, (int)Nn, inv_temp,
                       row_loss, row_correct);
  else
    hipLaunchKernelGGL(cs_kernel<float>, grid, dim3(CS_THREADS), 0, s, reinterpret_cast<const float*>(h),
                       reinterpret_cast<const float*>(q), ld, neg, neg_sb, neg_st, mask, rows, (int)T, (int)pd, (int)Nn, inv_temp,
                       row_loss, row_correct);
  return tmi_check_launch("tmi_contrastive_score");
}

extern "C" int tmi_contrastive_score(const void* h, const void* q, int64_t ld, int32_t dtype, const int32_t* neg, int64_t neg_sb,
                                     int64_t neg_st, const float* mask, float* row_loss, int32_t* row_correct, int64_t B, int64_t T,
                                     int64_t pd, int64_t Nn, float temperature, void* stream) {
  return tmi_plan_run<tmi_contrastive_score_impl>(h, q, ld, dtype, neg, neg_sb, neg_st, mask, row_loss, row_correct, B, T, pd, Nn,
                                                  temperature, stream);
}

static int tmi_vq_count_impl(const int32_t* idx, const float* mask, int64_t* counts, int64_t rows, int64_t G, int64_t Nc,
                             void* stream) {
  if (!idx || !counts || !tmi_aligned(idx, 4) || !tmi_aligned(mask, 4) || !tmi_aligned(counts, 8) || rows < 1 || rows > ((int64_t)1 << 30) ||
      G < 1 || Nc < 1 || G > 8192 || Nc > 8192 || G * Nc > 8192) {
    tmi_set_error("tmi_vq_count: bad argument");
    return TMI_ERR_INVALID;
  }
  // (a workgroup's LDS bins are 32 bit: at most 2^30 items each)
  const int64_t total = rows * G;
  int64_t blocks = (total + 2047) / 2048;
  if (blocks > 1024) blocks = 1024;
  const int64_t need = (total + ((int64_t)1 << 30) - 1) >> 30;
  if (blocks < need) blocks = need;
  hipLaunchKernelGGL(vq_count_kernel, dim3((unsigned)blocks), dim3(256), (size_t)(G * Nc) * sizeof(uint32_t),
                     reinterpret_cast<hipStream_t>(stream), idx, mask, reinterpret_cast<unsigned long long*>(counts), rows, (int)G,
                     (int)Nc);
  return tmi_check_launch("tmi_vq_count");
}

extern "C" int tmi_vq_count(const int32_t* idx, const float* mask, int64_t* counts, int64_t rows, int64_t G, int64_t Nc,
                            void* stream) {
  return tmi_plan_run<tmi_vq_count_impl>(idx, mask, counts, rows, G, Nc, stream);
}
