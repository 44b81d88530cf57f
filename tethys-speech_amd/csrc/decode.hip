// Greedy decoding's LM head: tmi_lm_head_argmax (W:675 / W:697: argmax(lm_head(decoder_out)[:, -1, :])).
//
// One launch per decoding step does what would otherwise be the final decoder LayerNorm, a [B*t, d] x [d, 51904] logits
// GEMM over the whole prefix and an argmax over the B last rows: only the M rows that are decoded are normalised (in the
// prologue, fp32) and multiplied, and the logits never reach memory.
//
// Form (cdna_hip_programming.md, "GEMV / M <= 16 decode weights"): the LM head is streamed ONCE per step straight into
// VGPRs - no LDS staging - with nontemporal 16-byte loads, two chunks of U rows in flight per thread.  A 256-thread workgroup
// owns 128 columns: lane & 15 picks 8 consecutive columns, the 16 (wave, lane >> 4) pairs split the d rows of the head
// (row k belongs to slice k % 16), so a wave reads four whole 256-byte row segments per load (bf16).  The normalised
// rows sit in LDS as [d][MT] fp32, so one row step reads its MT activations with MT/4 16-byte LDS reads (a broadcast: the
// wave touches four rows).  Partials are folded in a fixed order (two butterflies inside the wave, then the four waves
// through LDS), so every logit is computed the same way in every run.
//
// Cross-workgroup argmax: each workgroup's best column per row becomes a 64-bit key (order-preserving float bits << 32 |
// ~column) and joins the row's slot with an agent-scope 64-bit atomic max - the largest logit wins, and among equal logits
// the smallest column (tf.argmax).  Max is order-independent, so the result does not depend on which workgroup arrives
// first.  The last workgroup to finish (an agent-scope completion counter) publishes the ids and the EOS count and puts the
// slots and the counter back to zero: the workspace is clean again for the next launch, with no memset per step.
#include "tmi_common.h"
#include <string>
#include <type_traits>

namespace {

constexpr int AM_THREADS = 256;
constexpr int AM_COLS = 128;      // columns per workgroup: 16 column groups of 8
constexpr int AM_KSLICES = 16;    // row slices per workgroup

// Decode constraints (tmi_lm_head_*_c; the rule is include/tethys_mi.h's "Decode constraints"): two bit sets per row,
// column n at bit n & 31 of word n >> 5.  A thread of the epilogue owns 8 consecutive columns from a multiple of 8, so its
// bits are one byte of one word of each set.  C = false compiles all of it away: the unconstrained kernels are unchanged.
struct am_cons {
  const uint32_t* seen;
  const uint32_t* banned;
  int64_t bits_ld;
  float penalty;
};
template <bool C>
__device__ __forceinline__ void am_cons_bits(const am_cons& cs, int r, int c0, int V, uint32_t& sb, uint32_t& bb) {
  sb = 0, bb = 0;
  if constexpr (C) {
    if (c0 < V) {  // (a word at or past ceil(V / 32) is never read)
      const int64_t o = (int64_t)r * cs.bits_ld + (c0 >> 5);
      if (cs.seen) sb = (cs.seen[o] >> (c0 & 31)) & 0xffu;
      if (cs.banned) bb = (cs.banned[o] >> (c0 & 31)) & 0xffu;
    }
  }
}
// z -> z': -inf when banned, z / penalty (z > 0) or z * penalty (z <= 0) when seen
template <bool C>
__device__ __forceinline__ float am_cons_logit(float z, uint32_t sb, uint32_t bb, int c, float penalty) {
  if constexpr (C) {
    if ((bb >> c) & 1u) return -INFINITY;
    if ((sb >> c) & 1u) return z > 0.f ? __fdiv_rn(z, penalty) : z * penalty;
  }
  return z;
}

template <typename TW> struct am_rows;
// 8 consecutive columns of one weight row, in registers
template <> struct am_rows<bf16_t> {
  static constexpr int U = 8;  // rows per chunk (two chunks in flight: 2 x 8 x 16 B per thread)
  u32x4 r;
  __device__ __forceinline__ void load(const bf16_t* p) { r = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
  __device__ __forceinline__ float get(int c) const {
    const uint32_t w = r[c >> 1];
    return __uint_as_float((c & 1) ? (w & 0xffff0000u) : (w << 16));
  }
};
template <> struct am_rows<float> {
  static constexpr int U = 4;
  u32x4 r0, r1;
  __device__ __forceinline__ void load(const float* p) {
    r0 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
    r1 = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p) + 1);
  }
  __device__ __forceinline__ float get(int c) const { return __uint_as_float(c < 4 ? r0[c] : r1[c - 4]); }
};

template <int MT>
__device__ __forceinline__ void am_fma_row(float (&acc)[MT][8], const float* __restrict__ xk, const float (&w)[8]) {
#pragma unroll
  for (int m = 0; m < MT; m += (MT >= 4 ? 4 : 1)) {
    if constexpr (MT >= 4) {
      const f32x4 xv = *reinterpret_cast<const f32x4*>(xk + m);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[m + q][c] = fmaf(xv[q], w[c], acc[m + q][c]);
    } else {
      const float xv = xk[m];
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[m][c] = fmaf(xv, w[c], acc[m][c]);
    }
  }
}

// The shared body of the LM-head kernels: rows [row0, row0 + rows) of workgroup (blockIdx.x, blockIdx.y) times the
// workgroup's 128 columns of the head, left in LDS as the four waves' partials red[(wave * MT + m) * 128 + column]
// (fold them as ((red0 + red1) + red2) + red3).  Ends with every thread past a barrier.
template <typename TW, int MT>
__device__ __forceinline__ void am_head_tile(float* am_lds, const void* __restrict__ xv, int64_t x_ld, int x_bf16,
                                             const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                             const TW* __restrict__ w, int64_t w_ld, int d, int V, int row0, int rows) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // ---- prologue: rows [row0, row0 + rows) normalised (or copied) into LDS as xs[k * MT + m], fp32
  float* xs = am_lds;
  for (int m = wave; m < MT; m += 4) {
    if (m >= rows) {
      for (int k = lane; k < d; k += 64) xs[k * MT + m] = 0.f;
      continue;
    }
    const int64_t base = (int64_t)(row0 + m) * x_ld;
    auto ld = [&](int k) -> float {
      return x_bf16 ? (float)reinterpret_cast<const bf16_t*>(xv)[base + k] : reinterpret_cast<const float*>(xv)[base + k];
    };
    if (gamma) {
      float s = 0.f;
      for (int k = lane; k < d; k += 64) s += ld(k);
      const float mean = wave_sum(s) / (float)d;
      float q = 0.f;
      for (int k = lane; k < d; k += 64) {
        const float c = ld(k) - mean;
        q += c * c;
      }
      const float rstd = rsqrtf(wave_sum(q) / (float)d + eps);
      for (int k = lane; k < d; k += 64) xs[k * MT + m] = (ld(k) - mean) * rstd * gamma[k] + beta[k];
    } else {
      for (int k = lane; k < d; k += 64) xs[k * MT + m] = ld(k);
    }
  }
  __syncthreads();

  // ---- stream the weights: this thread's 8 columns, rows ks, ks + 16, ...
  const int cg = lane & 15, ks = wave * 4 + (lane >> 4);
  const int col0 = blockIdx.x * AM_COLS + cg * 8;
  const bool live = col0 < V;  // (w_ld >= V and both multiples of 8: a live group's 8 columns are inside the row)
  const TW* wp = w + (int64_t)ks * w_ld + col0;
  const int64_t wstep = (int64_t)AM_KSLICES * w_ld;
  float acc[MT][8];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[m][c] = 0.f;

  constexpr int U = am_rows<TW>::U;
  const int nk = ks < d ? (d - ks + AM_KSLICES - 1) / AM_KSLICES : 0;  // rows of this slice
  const int nchunks = live ? nk / U : 0;
  am_rows<TW> cur[U], nxt[U];
  if (nchunks > 0) {
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u].load(wp + u * wstep);
  }
  for (int ch = 0; ch < nchunks; ++ch) {
    if (ch + 1 < nchunks) {
      const TW* p = wp + (int64_t)(ch + 1) * U * wstep;
#pragma unroll
      for (int u = 0; u < U; ++u) nxt[u].load(p + u * wstep);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float wv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) wv[c] = cur[u].get(c);
      am_fma_row<MT>(acc, xs + (int64_t)(ks + (ch * U + u) * AM_KSLICES) * MT, wv);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = nxt[u];
  }
  if (live) {  // the slice's last nk % U rows
    for (int j = nchunks * U; j < nk; ++j) {
      am_rows<TW> r;
      r.load(wp + j * wstep);
      float wv[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) wv[c] = r.get(c);
      am_fma_row<MT>(acc, xs + (int64_t)(ks + j * AM_KSLICES) * MT, wv);
    }
  }

  // ---- fold the 16 slices: the wave's four (lane >> 4 = 0..3, butterfly), then the four waves through LDS in order
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      float v = acc[m][c];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      acc[m][c] = v;
    }
  __syncthreads();  // (every wave is done with xs: the fold reuses the LDS)
  float* red = am_lds;  // [4][MT][128]
  if (lane < 16) {
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
      for (int c = 0; c < 8; ++c) red[(wave * MT + m) * AM_COLS + cg * 8 + c] = acc[m][c];
  }
  __syncthreads();
}

// grid (ceil(V / 128), ceil(M / MT)); dynamic LDS max(d * MT, 4 * MT * 128) floats
template <typename TW, int MT, bool C>
__device__ __forceinline__ void lm_head_argmax_body(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, int32_t* __restrict__ ids, int64_t ids_ld,
    int eos_id, int32_t* __restrict__ eos_count, uint64_t* __restrict__ slots, uint32_t* __restrict__ counter,
    const am_cons cs) {
  extern __shared__ __attribute__((aligned(16))) float am_lds[];
  __shared__ int am_last, am_eos;
  const int tid = threadIdx.x;
  const int row0 = blockIdx.y * MT;
  const int rows = min(MT, M - row0);
  am_head_tile<TW, MT>(am_lds, xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, d, V, row0, rows);
  const float* red = am_lds;

  // ---- per row: best key over the workgroup's 128 columns (16 lanes of 8 columns), one atomic max per row
  {
    const int m = tid >> 4, g = tid & 15;
    uint64_t best = 0;  // 0 = no candidate (every real key is larger: its ~column half is nonzero or its value half is)
    if (m < rows) {
      const int c0 = blockIdx.x * AM_COLS + g * 8;
      uint32_t sb, bb;
      am_cons_bits<C>(cs, row0 + m, c0, V, sb, bb);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int col = c0 + c;
        const int o = m * AM_COLS + g * 8 + c;
        const float z = ((red[o] + red[MT * AM_COLS + o]) + red[2 * MT * AM_COLS + o]) + red[3 * MT * AM_COLS + o];
        const float v = am_cons_logit<C>(z, sb, bb, c, cs.penalty);
        const uint64_t key = ((uint64_t)am_order(v) << 32) | (uint64_t)(~(uint32_t)col);
        if (col < V && key > best) best = key;
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const uint64_t other = __shfl_xor(best, o, 64);
      best = other > best ? other : best;
    }
    if (m < rows && g == 0 && best != 0)
      __hip_atomic_fetch_max(slots + row0 + m, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  // ---- completion: the last workgroup publishes and cleans up
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const uint32_t total = gridDim.x * gridDim.y;
    const uint32_t prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    am_last = prev == total - 1;
    am_eos = 0;
  }
  __syncthreads();
  if (!am_last) return;
  __threadfence();
  int n_eos = 0;
  for (int r = tid; r < M; r += AM_THREADS) {
    const uint64_t key = __hip_atomic_load(slots + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int32_t id = (int32_t)(~(uint32_t)key);
    ids[(int64_t)r * ids_ld] = id;
    n_eos += (eos_id >= 0 && id == eos_id);
    __hip_atomic_store(slots + r, (uint64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (n_eos) atomicAdd(&am_eos, n_eos);
  __syncthreads();
  if (tid == 0) {
    if (eos_count) eos_count[0] = am_eos;
    __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_argmax_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, int32_t* __restrict__ ids, int64_t ids_ld,
    int eos_id, int32_t* __restrict__ eos_count, uint64_t* __restrict__ slots, uint32_t* __restrict__ counter) {
  lm_head_argmax_body<TW, MT, false>(xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, M, d, V, ids, ids_ld, eos_id, eos_count,
                                     slots, counter, am_cons{nullptr, nullptr, 0, 1.f});
}
template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_argmax_c_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, int32_t* __restrict__ ids, int64_t ids_ld,
    int eos_id, int32_t* __restrict__ eos_count, uint64_t* __restrict__ slots, uint32_t* __restrict__ counter,
    const uint32_t* __restrict__ seen, const uint32_t* __restrict__ banned, int64_t bits_ld, float penalty) {
  lm_head_argmax_body<TW, MT, true>(xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, M, d, V, ids, ids_ld, eos_id, eos_count,
                                    slots, counter, am_cons{seen, banned, bits_ld, penalty});
}

// ---------------------------------------------------------------------------------------------------------------------
// Beam search's LM head: tmi_lm_head_topk.  The argmax kernel's body (am_head_tile) with a top-N epilogue: per row, the
// logsumexp of s = z * inv_temperature over the V real columns and the N largest s (ties: smaller column first), written
// as log-probabilities s - logsumexp.
//
// Per workgroup and row: (max, sum exp(s - max)) over its 128 columns (16 lanes, a fixed butterfly) and its N best keys
// (the argmax kernel's 64-bit keys, extracted in N rounds of a 16-lane max), both stored in the row's slots for this
// workgroup - plain stores, nothing depends on the arrival order.  The last workgroup of a row tile (one completion
// counter per tile) then works one wave per row: it folds the (max, sum) slots in a fixed order (lane w takes slots w,
// w + 64, ... in order, then a butterfly that pairs the lower lane first), takes tau = the N-th largest of the
// workgroups' best keys (N rounds of a wave max over the lists' heads held in registers), gathers the listed keys >= tau
// into LDS - they can only come from the N workgroups whose best key is >= tau, so there are at most N * N <= 256 - ranks
// them (rank = how many gathered keys are larger), writes the N best and puts every slot back to zero.
constexpr int TK_CAP = 256;    // gathered keys per row: N * N at most
constexpr int TK_HEADS = 8;    // list heads per lane: ceil(V / 128) <= 512

__device__ __forceinline__ float tk_unorder(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

__device__ __forceinline__ uint64_t tk_wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t other = __shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}

// grid (ceil(V / 128), ceil(M / MT)); dynamic LDS max(d * MT, 4 * MT * 128, 4 * TK_CAP * 2) floats
template <typename TW, int MT, bool C>
__device__ __forceinline__ void lm_head_topk_body(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, float inv_t, int N, int32_t* __restrict__ out_ids,
    float* __restrict__ out_lp, float* __restrict__ out_lse, uint32_t* __restrict__ counters, float2* __restrict__ part,
    uint64_t* __restrict__ keys, const am_cons cs) {
  extern __shared__ __attribute__((aligned(16))) float am_lds[];
  __shared__ int tk_last;
  __shared__ int tk_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * MT;
  const int rows = min(MT, M - row0);
  const int nwg = gridDim.x;
  am_head_tile<TW, MT>(am_lds, xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, d, V, row0, rows);
  const float* red = am_lds;

  // ---- per row (16 lanes of 8 columns): the (max, sum) partial and the workgroup's N best keys
  {
    const int m = tid >> 4, g = tid & 15;
    if (m < rows) {
      const int r = row0 + m;
      const int c0 = blockIdx.x * AM_COLS + g * 8;
      float s[8];
      uint64_t k8[8];
      float mx = -INFINITY;
      uint32_t sb, bb;
      am_cons_bits<C>(cs, r, c0, V, sb, bb);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int o = m * AM_COLS + g * 8 + c;
        const float z = ((red[o] + red[MT * AM_COLS + o]) + red[2 * MT * AM_COLS + o]) + red[3 * MT * AM_COLS + o];
        s[c] = am_cons_logit<C>(z, sb, bb, c, cs.penalty) * inv_t;
        const bool ok = c0 + c < V;
        // (a banned column keeps its key, value -inf: it ranks below every other column and is outside the logsumexp)
        k8[c] = ok ? (((uint64_t)am_order(s[c]) << 32) | (uint64_t)(~(uint32_t)(c0 + c))) : 0;
        if (ok && !((bb >> c) & 1u)) mx = fmaxf(mx, s[c]);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if constexpr (C)
          se += (c0 + c < V && !((bb >> c) & 1u) && mx > -INFINITY) ? expf(s[c] - mx) : 0.f;
        else
          se += (c0 + c < V) ? expf(s[c] - mx) : 0.f;
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) se += __shfl_xor(se, o, 64);  // (xor pairs: both lanes add the same two values)
      if (g == 0) part[(int64_t)r * nwg + blockIdx.x] = make_float2(mx, se);

      // N rounds: the best remaining key of the 128 columns goes to lane `round` (0 once the columns run out)
      uint64_t mine = 0;
      for (int round = 0; round < N; ++round) {
        uint64_t best = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) best = k8[c] > best ? k8[c] : best;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const uint64_t other = __shfl_xor(best, o, 64);
          best = other > best ? other : best;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) k8[c] = k8[c] == best ? 0 : k8[c];
        if (round == g) mine = best;
      }
      if (g < N) keys[((int64_t)r * nwg + blockIdx.x) * N + g] = mine;
    }
  }

  // ---- completion: the last workgroup of the row tile publishes and cleans up
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(counters + blockIdx.y, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    tk_last = prev == (uint32_t)nwg - 1;
  }
  __syncthreads();
  if (!tk_last) return;
  __threadfence();
  uint64_t* lk = reinterpret_cast<uint64_t*>(am_lds) + wave * TK_CAP;  // this wave's gathered keys
  for (int m = wave; m < rows; m += 4) {
    const int r = row0 + m;
    uint64_t* list = keys + (int64_t)r * nwg * N;
    uint64_t head[TK_HEADS];
#pragma unroll
    for (int i = 0; i < TK_HEADS; ++i) {
      const int wg = lane + 64 * i;
      head[i] = wg < nwg ? list[(int64_t)wg * N] : 0;
    }
    // logsumexp: fixed order, whatever the arrival order was
    float am = -INFINITY, as = 0.f;
    for (int wg = lane; wg < nwg; wg += 64) {
      float2* p = part + (int64_t)r * nwg + wg;
      const float2 v = *p;
      lse_fold(am, as, v.x, v.y);
      *p = make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float om = __shfl_xor(am, o, 64), os = __shfl_xor(as, o, 64);
      if (lane & o) {  // the lower lane's pair first, in both lanes
        float lm = om, ls = os;
        lse_fold(lm, ls, am, as);
        am = lm, as = ls;
      } else {
        lse_fold(am, as, om, os);
      }
    }
    const float lse = am + logf(as);
    if (out_lse && lane == 0) out_lse[r] = lse;

    // tau: the N-th largest head (0 when fewer than N workgroups: then every listed key is gathered)
    uint64_t tau = 0;
    {
      uint64_t h[TK_HEADS];
#pragma unroll
      for (int i = 0; i < TK_HEADS; ++i) h[i] = head[i];
      for (int round = 0; round < N; ++round) {
        uint64_t best = 0;
#pragma unroll
        for (int i = 0; i < TK_HEADS; ++i) best = h[i] > best ? h[i] : best;
        best = tk_wave_max(best);
#pragma unroll
        for (int i = 0; i < TK_HEADS; ++i) h[i] = h[i] == best ? 0 : h[i];
        tau = best;
      }
    }
    // gather the keys >= tau of the (at most N) lists whose head is >= tau
    if (lane == 0) tk_n[wave] = 0;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int i = 0; i < TK_HEADS; ++i) {
      const int wg = lane + 64 * i;
      if (head[i] != 0 && head[i] >= tau) {
        for (int j = 0; j < N; ++j) {
          const uint64_t key = list[(int64_t)wg * N + j];
          if (key == 0 || key < tau) break;  // (a list is sorted)
          lk[atomicAdd(&tk_n[wave], 1)] = key;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int c = tk_n[wave];
    for (int j = lane; j < c; j += 64) {
      const uint64_t key = lk[j];
      int rank = 0;
      for (int i = 0; i < c; ++i) rank += lk[i] > key;
      if (rank < N) {
        out_ids[(int64_t)r * N + rank] = (int32_t)(~(uint32_t)key);
        const float sv = tk_unorder((uint32_t)(key >> 32));
        if constexpr (C)  // (a banned column: -inf, also in a row whose every column is banned, where lse is -inf too)
          out_lp[(int64_t)r * N + rank] = sv == -INFINITY ? -INFINITY : sv - lse;
        else
          out_lp[(int64_t)r * N + rank] = sv - lse;
      }
    }
    for (int64_t j = lane; j < (int64_t)nwg * N; j += 64) list[j] = 0;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (lk and tk_n are reused by the wave's next row)
  }
  __syncthreads();
  if (tid == 0) __hip_atomic_store(counters + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_topk_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, float inv_t, int N, int32_t* __restrict__ out_ids,
    float* __restrict__ out_lp, float* __restrict__ out_lse, uint32_t* __restrict__ counters, float2* __restrict__ part,
    uint64_t* __restrict__ keys) {
  lm_head_topk_body<TW, MT, false>(xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, M, d, V, inv_t, N, out_ids, out_lp, out_lse,
                                   counters, part, keys, am_cons{nullptr, nullptr, 0, 1.f});
}
template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_topk_c_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, float inv_t, int N, int32_t* __restrict__ out_ids,
    float* __restrict__ out_lp, float* __restrict__ out_lse, uint32_t* __restrict__ counters, float2* __restrict__ part,
    uint64_t* __restrict__ keys, const uint32_t* __restrict__ seen, const uint32_t* __restrict__ banned, int64_t bits_ld,
    float penalty) {
  lm_head_topk_body<TW, MT, true>(xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, M, d, V, inv_t, N, out_ids, out_lp, out_lse,
                                  counters, part, keys, am_cons{seen, banned, bits_ld, penalty});
}

// ---------------------------------------------------------------------------------------------------------------------
// Sampled decoding's LM head: tmi_lm_head_sample.  The same body again (am_head_tile) with a choice rule on top; the rule
// is include/tethys_mi.h's.  The keys carry z, not z / temperature: dividing by a positive temperature keeps the order and
// can only merge neighbours, so ranking on z is the finer order - and top_k = 1 is the argmax kernel's token at every
// temperature.
//
// top_k >= 1.  Per workgroup and row: the (max, sum) partial of s = z / temperature and the top_k best keys of its 128
// columns (the top-k kernel's rounds; lane g keeps rounds g, g + 16, g + 32, g + 48), plain stores into the row's slots.
// The last workgroup of a row tile works one wave per row: the logsumexp fold of the top-k kernel; tau = the top_k-th
// largest list head by a radix select over the heads in registers (64 ballots of 8 compares: no cross-lane traffic);
// the at most top_k lists whose head is >= tau - no other list can hold one of the top_k keys - get one lane each; a
// top_k-round tournament over those lanes' heads (a wave max per round; the winner's lane pops its list, which it holds
// four keys at a time) leaves candidate j in lane j, so nothing like the top-k kernel's N * N gather exists at 64.
// Then p_j = exp(s_j - lse), the running sums in index order (through LDS: lane j adds p_0 .. p_j itself, one order for
// every lane), the nucleus size and the inverse-CDF draw as two ballots.
//
// top_k == 0 (Gumbel-max over the whole vocabulary).  Per workgroup and row: the (max, sum) partial, and the best key of
// s + g over its columns together with that column's unperturbed s (list slots 0 and 1).  The last workgroup takes the
// largest key - a max, so the arrival order cannot matter - and writes s - lse of its column.
//
// The last workgroup of the LAST tile to finish (a second counter) counts the finished rows.
constexpr int SM_MAXK = 64;

__device__ __forceinline__ uint64_t sm_key(float z, int col) {
  return ((uint64_t)am_order(z) << 32) | (uint64_t)(~(uint32_t)col);
}

// -log(u) of the uniform u = (n + 0.5) * 2^-24, n < 2^24.  u has 25 significant bits from n = 2^23 on, where fp32 would
// round it (n = 2^24 - 1 to 1.0: an infinite Gumbel); there 1 - u = (2^24 - 1 - n + 0.5) * 2^-24 is exact instead.
__device__ __forceinline__ float sm_neglog_u(uint32_t n) {
  if (n < (1u << 23)) return -logf(((float)n + 0.5f) * 0x1p-24f);
  return -log1pf(-(((float)(0xFFFFFFu - n) + 0.5f) * 0x1p-24f));
}

// grid (ceil(V / 128), ceil(M / MT)); dynamic LDS max(d * MT, 4 * MT * 128, 512) floats
template <typename TW, int MT, bool C>
__device__ __forceinline__ void lm_head_sample_body(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, float temperature, int top_k, float top_p,
    uint32_t stream_key, int suppress_id, int eos_id, int pad_id, int32_t* __restrict__ finished, int32_t* __restrict__ ids,
    int64_t ids_ld, float* __restrict__ out_lp, int32_t* __restrict__ n_finished, uint32_t* __restrict__ counters,
    float2* __restrict__ part, uint64_t* __restrict__ keys, const am_cons cs) {
  extern __shared__ __attribute__((aligned(16))) float am_lds[];
  __shared__ int sm_last, sm_count;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * MT;
  const int rows = min(MT, M - row0);
  const int nwg = gridDim.x;
  const int KL = top_k > 0 ? top_k : 2;  // list slots per (row, workgroup)
  am_head_tile<TW, MT>(am_lds, xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, d, V, row0, rows);
  const float* red = am_lds;

  // ---- per row (16 lanes of 8 columns): the (max, sum) partial and the workgroup's list
  {
    const int m = tid >> 4, g = tid & 15;
    if (m < rows) {
      const int r = row0 + m;
      const int c0 = blockIdx.x * AM_COLS + g * 8;
      float s[8];
      uint64_t k8[8];
      bool ok[8];
      float mx = -INFINITY;
      uint32_t sb, bb;
      am_cons_bits<C>(cs, r, c0, V, sb, bb);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int o = m * AM_COLS + g * 8 + c;
        const float z = am_cons_logit<C>(
            ((red[o] + red[MT * AM_COLS + o]) + red[2 * MT * AM_COLS + o]) + red[3 * MT * AM_COLS + o], sb, bb, c, cs.penalty);
        s[c] = __fdiv_rn(z, temperature);
        ok[c] = c0 + c < V && c0 + c != suppress_id && !((bb >> c) & 1u);  // (a banned column: one more suppressed id)
        k8[c] = ok[c] ? sm_key(z, c0 + c) : 0;
        if (ok[c]) mx = fmaxf(mx, s[c]);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) se += (ok[c] && mx > -INFINITY) ? expf(s[c] - mx) : 0.f;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) se += __shfl_xor(se, o, 64);  // (xor pairs: both lanes add the same two values)
      if (g == 0) part[(int64_t)r * nwg + blockIdx.x] = make_float2(mx, se);
      uint64_t* list = keys + ((int64_t)r * nwg + blockIdx.x) * KL;

      if (top_k > 0) {
        // top_k rounds: the best remaining key goes to lane round % 16, slot round / 16 (0 once the columns run out)
        uint64_t mine[SM_MAXK / 16] = {0, 0, 0, 0};
        bool more = true;
#pragma unroll
        for (int q = 0; q < SM_MAXK / 16; ++q) {
          for (int rr = 0; rr < 16 && more && q * 16 + rr < top_k; ++rr) {
            uint64_t best = 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) best = k8[c] > best ? k8[c] : best;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
              const uint64_t other = __shfl_xor(best, o, 64);
              best = other > best ? other : best;
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) k8[c] = k8[c] == best ? 0 : k8[c];
            if (rr == g) mine[q] = best;
            more = best != 0;  // (the same in all 16 lanes)
          }
        }
#pragma unroll
        for (int q = 0; q < SM_MAXK / 16; ++q)
          if (q * 16 + g < top_k) list[q * 16 + g] = mine[q];
      } else {
        const tmi_rowkey rk = tmi_row_key(stream_key, (uint32_t)r);
        uint64_t best = 0;
        float best_s = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          if (!ok[c]) continue;
          const float gum = -logf(sm_neglog_u(tmi_sample_bits(rk, (uint32_t)(c0 + c)) >> 8));
          const uint64_t key = sm_key(s[c] + gum, c0 + c);
          if (key > best) best = key, best_s = s[c];
        }
        uint64_t all = best;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const uint64_t other = __shfl_xor(all, o, 64);
          all = other > all ? other : all;
        }
        if (all != 0 && all == best) {  // (keys are distinct: one lane)
          list[0] = best;
          list[1] = (uint64_t)__float_as_uint(best_s);
        }
      }
    }
  }

  // ---- completion: the last workgroup of the row tile publishes and cleans up
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(counters + blockIdx.y, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    sm_last = prev == (uint32_t)nwg - 1;
  }
  __syncthreads();
  if (!sm_last) return;
  __threadfence();
  int* sl = reinterpret_cast<int*>(am_lds) + wave * 128;  // this wave's live lists ...
  float* pl = am_lds + wave * 128 + 64;                   // ... and its candidates' probabilities
  for (int m = wave; m < rows; m += 4) {
    const int r = row0 + m;
    uint64_t* list = keys + (int64_t)r * nwg * KL;
    uint64_t head[TK_HEADS];
#pragma unroll
    for (int i = 0; i < TK_HEADS; ++i) {
      const int wg = lane + 64 * i;
      head[i] = wg < nwg ? list[(int64_t)wg * KL] : 0;
    }
    // logsumexp: fixed order, whatever the arrival order was (the top-k kernel's fold)
    float am = -INFINITY, as = 0.f;
    for (int wg = lane; wg < nwg; wg += 64) {
      float2* p = part + (int64_t)r * nwg + wg;
      const float2 v = *p;
      lse_fold(am, as, v.x, v.y);
      *p = make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float om = __shfl_xor(am, o, 64), os = __shfl_xor(as, o, 64);
      if (lane & o) {  // the lower lane's pair first, in both lanes
        float lm = om, ls = os;
        lse_fold(lm, ls, am, as);
        am = lm, as = ls;
      } else {
        lse_fold(am, as, om, os);
      }
    }
    const float lse = am + logf(as);
    const bool was_finished = finished[r] != 0;
    int token = pad_id;
    float lp = 0.f;

    if (was_finished) {
      // (nothing to choose; the slots are still cleaned below)
    } else if (top_k == 0) {
      uint64_t best = 0;
#pragma unroll
      for (int i = 0; i < TK_HEADS; ++i) best = head[i] > best ? head[i] : best;
      const uint64_t all = tk_wave_max(best);
      float s_tok = 0.f;
#pragma unroll
      for (int i = 0; i < TK_HEADS; ++i)
        if (all != 0 && head[i] == all) s_tok = __uint_as_float((uint32_t)list[(int64_t)(lane + 64 * i) * KL + 1]);
      s_tok = wave_sum(s_tok);  // (one lane holds it, the others 0)
      if (all != 0) {  // (0: no column can be drawn - V == 1 and it is suppressed - and the row writes pad, as below)
        token = (int32_t)(~(uint32_t)all);
        lp = s_tok - lse;
      }
    } else {
      // tau: the top_k-th largest head (0 when fewer lists than that have a key)
      uint64_t tau = 0;
      for (int b = 63; b >= 0; --b) {
        const uint64_t cand = tau | ((uint64_t)1 << b);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < TK_HEADS; ++i) cnt += __popcll(__ballot(head[i] >= cand));
        if (cnt >= top_k) tau = cand;
      }
      // one lane per live list (at most top_k <= 64 of them)
      int nlive = 0;
#pragma unroll
      for (int i = 0; i < TK_HEADS; ++i) {
        const bool live = head[i] != 0 && head[i] >= tau;
        const uint64_t mask = __ballot(live);
        if (live) sl[nlive + __popcll(mask & (((uint64_t)1 << lane) - 1))] = lane + 64 * i;
        nlive += __popcll(mask);
      }
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const uint64_t* mylist = list + (int64_t)(lane < nlive ? sl[lane] : 0) * KL;
      uint64_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;
      int pos = 0, have = 0;
      auto refill = [&]() {
        h0 = pos < KL ? mylist[pos] : 0;
        h1 = pos + 1 < KL ? mylist[pos + 1] : 0;
        h2 = pos + 2 < KL ? mylist[pos + 2] : 0;
        h3 = pos + 3 < KL ? mylist[pos + 3] : 0;
        pos += 4, have = 4;
      };
      if (lane < nlive) refill();
      uint64_t cand = 0;
      int kc = 0;  // candidates found: top_k, or every column that can be drawn when there are fewer
      for (; kc < top_k; ++kc) {
        const uint64_t best = tk_wave_max(h0);
        if (best == 0) break;
        if (lane == kc) cand = best;
        if (h0 == best) {
          h0 = h1, h1 = h2, h2 = h3, h3 = 0;
          if (--have == 0 && pos < KL) refill();
        }
      }
      // p_j = exp(s_j - lse), the running sums P_j in index order, the nucleus and the draw
      const float s_me = __fdiv_rn(tk_unorder((uint32_t)(cand >> 32)), temperature);
      pl[lane] = lane < kc ? expf(s_me - lse) : 0.f;
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      float P = 0.f;
      for (int j = 0; j < kc; ++j) P += j <= lane ? pl[j] : 0.f;
      const float p_all = __shfl(P, kc > 0 ? kc - 1 : 0, 64);
      int mnuc = kc;
      if (top_p < 1.f) {
        const uint64_t in = __ballot(lane < kc && P >= top_p * p_all);
        if (in) mnuc = __ffsll((unsigned long long)in);
      }
      const tmi_rowkey rk = tmi_row_key(stream_key, (uint32_t)r);
      const float u = ((float)(tmi_sample_bits(rk, 0xFFFFFFFFu) >> 8) + 0.5f) * 0x1p-24f;
      const float thr = u * __shfl(P, mnuc > 0 ? mnuc - 1 : 0, 64);
      const uint64_t hit = __ballot(lane < mnuc && P > thr);
      const int j = hit ? __ffsll((unsigned long long)hit) - 1 : (mnuc > 0 ? mnuc - 1 : 0);
      if (kc > 0) {  // (kc == 0: no column can be drawn - V == 1 and it is suppressed - and the row writes pad)
        token = (int32_t)(~(uint32_t)__shfl(cand, j, 64));
        lp = __shfl(s_me, j, 64) - lse;
      }
    }
    if (lane == 0) {
      ids[(int64_t)r * ids_ld] = token;
      if (out_lp) out_lp[r] = lp;
      if (!was_finished && token == eos_id) finished[r] = 1;
    }
    for (int64_t j = lane; j < (int64_t)nwg * KL; j += 64) list[j] = 0;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // (sl and pl are reused by the wave's next row)
  }

  // ---- the last tile to finish counts the finished rows
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    __hip_atomic_store(counters + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t prev = __hip_atomic_fetch_add(counters + M, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    sm_last = prev == gridDim.y - 1;
    sm_count = 0;
  }
  __syncthreads();
  if (!sm_last) return;
  __threadfence();
  int n = 0;
  for (int r = tid; r < M; r += AM_THREADS)
    n += __hip_atomic_load(finished + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
  if (n) atomicAdd(&sm_count, n);
  __syncthreads();
  if (tid == 0) {
    if (n_finished) n_finished[0] = sm_count;
    __hip_atomic_store(counters + M, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_sample_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, float temperature, int top_k, float top_p,
    uint32_t stream_key, int suppress_id, int eos_id, int pad_id, int32_t* __restrict__ finished, int32_t* __restrict__ ids,
    int64_t ids_ld, float* __restrict__ out_lp, int32_t* __restrict__ n_finished, uint32_t* __restrict__ counters,
    float2* __restrict__ part, uint64_t* __restrict__ keys) {
  lm_head_sample_body<TW, MT, false>(xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, M, d, V, temperature, top_k, top_p,
                                     stream_key, suppress_id, eos_id, pad_id, finished, ids, ids_ld, out_lp, n_finished,
                                     counters, part, keys, am_cons{nullptr, nullptr, 0, 1.f});
}
template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_sample_c_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, float temperature, int top_k, float top_p,
    uint32_t stream_key, int suppress_id, int eos_id, int pad_id, int32_t* __restrict__ finished, int32_t* __restrict__ ids,
    int64_t ids_ld, float* __restrict__ out_lp, int32_t* __restrict__ n_finished, uint32_t* __restrict__ counters,
    float2* __restrict__ part, uint64_t* __restrict__ keys, const uint32_t* __restrict__ seen,
    const uint32_t* __restrict__ banned, int64_t bits_ld, float penalty) {
  lm_head_sample_body<TW, MT, true>(xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, M, d, V, temperature, top_k, top_p,
                                    stream_key, suppress_id, eos_id, pad_id, finished, ids, ids_ld, out_lp, n_finished,
                                    counters, part, keys, am_cons{seen, banned, bits_ld, penalty});
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side: the one launch path of the six kernels above.

// What shapes a launch of any of them: the row tile, am_head_tile's LDS and the workgroups per row tile.
struct am_geom {
  int MT;              // rows per workgroup
  int64_t lds_floats;  // max(d * MT, 4 * MT * 128); a head whose epilogue needs more raises it
  int64_t nwg;         // ceil(V / 128)
};

// One instantiation's launch as entry point `name`.  Above 64 KiB of dynamic LDS (16 rows of d > 1024) a kernel has to opt
// in, up to what it needs (160 KiB per CU on gfx950, its few static bytes included); `opted` is this instantiation's own.
template <auto Kern, typename... A>
int am_launch_one(const char* name, dim3 grid, size_t lds, hipStream_t s, A... a) {
  static size_t opted = 65536;
  if (lds > opted) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess) {
      (void)hipGetLastError();
      tmi_set_error((std::string(name) + ": the LDS size could not be granted").c_str());
      return TMI_ERR_LAUNCH;
    }
    opted = lds;
  }
  hipLaunchKernelGGL(Kern, grid, dim3(AM_THREADS), lds, s, a...);
  return tmi_check_launch(name);
}

// A head's launch: KernC with the constraint's four arguments behind `a` when there is one, Kern otherwise.
template <auto Kern, auto KernC, typename... A>
int am_launch(const char* name, const char* name_c, const am_geom& g, int64_t M, void* stream, const am_cons* cs, A... a) {
  const dim3 grid((unsigned)g.nwg, (unsigned)((M + g.MT - 1) / g.MT));
  const size_t lds = (size_t)g.lds_floats * 4;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (cs) return am_launch_one<KernC>(name_c, grid, lds, s, a..., cs->seen, cs->banned, cs->bits_ld, cs->penalty);
  return am_launch_one<Kern>(name, grid, lds, s, a...);
}

// f(am_tag<TW>, integral_constant<MT>) for the weights' dtype and the row tile of a call
template <typename TW> struct am_tag { using type = TW; };
template <typename F>
int am_dispatch(int32_t w_dtype, int MT, F f) {
  auto tile = [&](auto tw) -> int {
    switch (MT) {
      case 1: return f(tw, std::integral_constant<int, 1>{});
      case 2: return f(tw, std::integral_constant<int, 2>{});
      case 4: return f(tw, std::integral_constant<int, 4>{});
      case 8: return f(tw, std::integral_constant<int, 8>{});
      case 16: return f(tw, std::integral_constant<int, 16>{});
    }
    return TMI_ERR_INVALID;
  };
  return w_dtype == TMI_BF16 ? tile(am_tag<bf16_t>{}) : tile(am_tag<float>{});
}

// What the three heads ask of the arguments they share -> g; false: a bad argument.
bool am_args(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta, const void* w, int64_t w_ld,
             int32_t w_dtype, int64_t M, int64_t d, int64_t V, const void* workspace, am_geom& g) {
  const bool dt_ok = (x_dtype == TMI_F32 || x_dtype == TMI_BF16) && (w_dtype == TMI_F32 || w_dtype == TMI_BF16);
  g.MT = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : M <= 8 ? 8 : 16;
  g.lds_floats = d * g.MT > 4 * g.MT * AM_COLS ? d * g.MT : 4 * g.MT * AM_COLS;
  g.nwg = (V + AM_COLS - 1) / AM_COLS;
  return x && w && workspace && dt_ok && M >= 1 && M <= (int64_t)16 * 65535 && d >= 1 && V >= 1 && w_ld >= V && !(w_ld & 7) &&
         tmi_aligned(w, 16) && x_ld >= d && (gamma == nullptr) == (beta == nullptr) && tmi_aligned(workspace, 8) &&
         g.lds_floats * 4 <= 160 * 1024 - 256;
}

}  // namespace

// The constraint arguments of the _c entry points -> the kernels' form, or false.  Both sets NULL is "no constraint": the
// unconstrained instantiation runs (cs stays null), which is what gives such a call the originals' bits.
static bool am_cons_args(const uint32_t* seen, const uint32_t* banned, int64_t bits_ld, float penalty, int64_t V, am_cons& c,
                         const am_cons*& cs) {
  cs = nullptr;
  if (!(penalty > 0.f && penalty < INFINITY)) return false;
  if (!seen && !banned) return true;
  if (bits_ld < (V + 31) / 32 || ((reinterpret_cast<uintptr_t>(seen) | reinterpret_cast<uintptr_t>(banned)) & 3)) return false;
  c = am_cons{seen, banned, bits_ld, penalty};
  cs = &c;
  return true;
}

static int am_run(const char* bad, const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                  float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V, int32_t* ids,
                  int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace, int64_t workspace_bytes, void* stream,
                  const am_cons* cs) {
  am_geom g;
  if (!am_args(x, x_ld, x_dtype, gamma, beta, w, w_ld, w_dtype, M, d, V, workspace, g) || !ids || V >= INT32_MAX ||
      ids_ld < 1 || workspace_bytes < 8 * (M + 1)) {
    tmi_set_error(bad);
    return TMI_ERR_INVALID;
  }
  uint64_t* slots = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* counter = reinterpret_cast<uint32_t*>(slots + M);
  const int xb = x_dtype == TMI_BF16;
  return am_dispatch(w_dtype, g.MT, [&](auto tw, auto mt) {
    using TW = typename decltype(tw)::type;
    return am_launch<lm_head_argmax_kernel<TW, mt()>, lm_head_argmax_c_kernel<TW, mt()>>(
        "tmi_lm_head_argmax", "tmi_lm_head_argmax_c", g, M, stream, cs, x, x_ld, xb, gamma, beta, eps,
        reinterpret_cast<const TW*>(w), w_ld, (int)M, (int)d, (int)V, ids, ids_ld, eos_id, eos_count, slots, counter);
  });
}
static int tmi_lm_head_argmax_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                   float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                   int32_t* ids, int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  return am_run("tmi_lm_head_argmax: bad argument", x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, ids, ids_ld,
                eos_id, eos_count, workspace, workspace_bytes, stream, nullptr);
}
extern "C" int tmi_lm_head_argmax(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                  float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                  int32_t* ids, int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  return tmi_plan_run<tmi_lm_head_argmax_impl>(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, ids, ids_ld,
                                               eos_id, eos_count, workspace, workspace_bytes, stream);
}
static int tmi_lm_head_argmax_c_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                     float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                     int32_t* ids, int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace,
                                     int64_t workspace_bytes, const uint32_t* seen, const uint32_t* banned, int64_t bits_ld,
                                     float penalty, void* stream) {
  am_cons c;
  const am_cons* cs;
  if (!am_cons_args(seen, banned, bits_ld, penalty, V, c, cs)) {
    tmi_set_error("tmi_lm_head_argmax_c: bad argument");
    return TMI_ERR_INVALID;
  }
  return am_run("tmi_lm_head_argmax_c: bad argument", x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, ids,
                ids_ld, eos_id, eos_count, workspace, workspace_bytes, stream, cs);
}
extern "C" int tmi_lm_head_argmax_c(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                    float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                    int32_t* ids, int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace,
                                    int64_t workspace_bytes, const uint32_t* seen, const uint32_t* banned, int64_t bits_ld,
                                    float penalty, void* stream) {
  return tmi_plan_run<tmi_lm_head_argmax_c_impl>(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, ids, ids_ld,
                                                 eos_id, eos_count, workspace, workspace_bytes, seen, banned, bits_ld,
                                                 penalty, stream);
}

static int tk_run(const char* bad, const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                  float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                  float inv_temperature, int64_t N, int32_t* ids, float* logprobs, float* lse, void* workspace,
                  int64_t workspace_bytes, void* stream, const am_cons* cs) {
  am_geom g;
  const bool shared_ok = am_args(x, x_ld, x_dtype, gamma, beta, w, w_ld, w_dtype, M, d, V, workspace, g);
  const int64_t nwg = g.nwg;
  if (!shared_ok || !ids || !logprobs || nwg > 64 * TK_HEADS || N < 1 || N > 16 || N > V ||
      !(inv_temperature > 0.f && inv_temperature < INFINITY) || workspace_bytes < 8 * M * (1 + nwg * (N + 1))) {
    tmi_set_error(bad);
    return TMI_ERR_INVALID;
  }
  if (g.lds_floats < 4 * TK_CAP * 2) g.lds_floats = 4 * TK_CAP * 2;  // (the gathered keys of the epilogue's four waves)
  char* base = reinterpret_cast<char*>(workspace);
  uint32_t* counters = reinterpret_cast<uint32_t*>(base);  // (one per row tile; 8 * M bytes reserved)
  float2* part = reinterpret_cast<float2*>(base + 8 * M);
  uint64_t* keys = reinterpret_cast<uint64_t*>(base + 8 * M + 8 * M * nwg);
  const int xb = x_dtype == TMI_BF16;
  return am_dispatch(w_dtype, g.MT, [&](auto tw, auto mt) {
    using TW = typename decltype(tw)::type;
    return am_launch<lm_head_topk_kernel<TW, mt()>, lm_head_topk_c_kernel<TW, mt()>>(
        "tmi_lm_head_topk", "tmi_lm_head_topk_c", g, M, stream, cs, x, x_ld, xb, gamma, beta, eps,
        reinterpret_cast<const TW*>(w), w_ld, (int)M, (int)d, (int)V, inv_temperature, (int)N, ids, logprobs, lse, counters,
        part, keys);
  });
}
static int tmi_lm_head_topk_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                 float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                 float inv_temperature, int64_t N, int32_t* ids, float* logprobs, float* lse,
                                 void* workspace, int64_t workspace_bytes, void* stream) {
  return tk_run("tmi_lm_head_topk: bad argument", x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V,
                inv_temperature, N, ids, logprobs, lse, workspace, workspace_bytes, stream, nullptr);
}
extern "C" int tmi_lm_head_topk(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                float inv_temperature, int64_t N, int32_t* ids, float* logprobs, float* lse, void* workspace,
                                int64_t workspace_bytes, void* stream) {
  return tmi_plan_run<tmi_lm_head_topk_impl>(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, inv_temperature, N,
                                             ids, logprobs, lse, workspace, workspace_bytes, stream);
}
static int tmi_lm_head_topk_c_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                   float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                   float inv_temperature, int64_t N, int32_t* ids, float* logprobs, float* lse,
                                   void* workspace, int64_t workspace_bytes, const uint32_t* seen, const uint32_t* banned,
                                   int64_t bits_ld, float penalty, void* stream) {
  am_cons c;
  const am_cons* cs;
  if (!am_cons_args(seen, banned, bits_ld, penalty, V, c, cs)) {
    tmi_set_error("tmi_lm_head_topk_c: bad argument");
    return TMI_ERR_INVALID;
  }
  return tk_run("tmi_lm_head_topk_c: bad argument", x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V,
                inv_temperature, N, ids, logprobs, lse, workspace, workspace_bytes, stream, cs);
}
extern "C" int tmi_lm_head_topk_c(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                  float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                  float inv_temperature, int64_t N, int32_t* ids, float* logprobs, float* lse,
                                  void* workspace, int64_t workspace_bytes, const uint32_t* seen, const uint32_t* banned,
                                  int64_t bits_ld, float penalty, void* stream) {
  return tmi_plan_run<tmi_lm_head_topk_c_impl>(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, inv_temperature,
                                               N, ids, logprobs, lse, workspace, workspace_bytes, seen, banned, bits_ld,
                                               penalty, stream);
}

extern "C" int64_t tmi_lm_head_sample_workspace_bytes(int64_t M, int64_t V, int64_t top_k) {
  if (M < 1 || V < 1 || top_k < 0 || top_k > SM_MAXK) return -1;
  const int64_t nwg = (V + AM_COLS - 1) / AM_COLS;
  return 8 * M * (1 + nwg * (1 + (top_k > 0 ? top_k : 2))) + 8;
}

static int sm_run(const char* bad, const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                  float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                  float temperature, int64_t top_k, float top_p, uint64_t seed, int32_t suppress_id, int32_t eos_id,
                  int32_t pad_id, int32_t* finished, int32_t* ids, int64_t ids_ld, float* logprob, int32_t* n_finished,
                  void* workspace, int64_t workspace_bytes, void* stream, const am_cons* cs) {
  am_geom g;
  const bool shared_ok = am_args(x, x_ld, x_dtype, gamma, beta, w, w_ld, w_dtype, M, d, V, workspace, g);
  const int64_t nwg = g.nwg;
  const bool rule_ok = temperature > 0.f && temperature < INFINITY && top_k >= 0 && top_k <= SM_MAXK && top_p > 0.f &&
                       top_p <= 1.f && (top_k > 0 || top_p == 1.f);
  if (!shared_ok || !ids || !finished || !n_finished || nwg > 64 * TK_HEADS || !rule_ok || ids_ld < 1 ||
      workspace_bytes < tmi_lm_head_sample_workspace_bytes(M, V, top_k)) {
    tmi_set_error(bad);
    return TMI_ERR_INVALID;
  }
  if (g.lds_floats < 512) g.lds_floats = 512;  // (the epilogue's four waves: 64 lists and 64 probabilities each)
  char* base = reinterpret_cast<char*>(workspace);
  uint32_t* counters = reinterpret_cast<uint32_t*>(base);  // (one per row tile, then the tiles' own at [M]; 8 * M + 8 bytes)
  float2* part = reinterpret_cast<float2*>(base + 8 * M + 8);
  uint64_t* keys = reinterpret_cast<uint64_t*>(base + 8 * M + 8 + 8 * M * nwg);
  const int xb = x_dtype == TMI_BF16;
  const uint32_t skey = tmi_stream_key(seed, 0);
  return am_dispatch(w_dtype, g.MT, [&](auto tw, auto mt) {
    using TW = typename decltype(tw)::type;
    return am_launch<lm_head_sample_kernel<TW, mt()>, lm_head_sample_c_kernel<TW, mt()>>(
        "tmi_lm_head_sample", "tmi_lm_head_sample_c", g, M, stream, cs, x, x_ld, xb, gamma, beta, eps,
        reinterpret_cast<const TW*>(w), w_ld, (int)M, (int)d, (int)V, temperature, (int)top_k, top_p, skey, (int)suppress_id,
        (int)eos_id, (int)pad_id, finished, ids, ids_ld, logprob, n_finished, counters, part, keys);
  });
}
static int tmi_lm_head_sample_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                   float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                   float temperature, int64_t top_k, float top_p, uint64_t seed, int32_t suppress_id,
                                   int32_t eos_id, int32_t pad_id, int32_t* finished, int32_t* ids, int64_t ids_ld,
                                   float* logprob, int32_t* n_finished, void* workspace, int64_t workspace_bytes,
                                   void* stream) {
  return sm_run("tmi_lm_head_sample: bad argument", x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, temperature,
                top_k, top_p, seed, suppress_id, eos_id, pad_id, finished, ids, ids_ld, logprob, n_finished, workspace,
                workspace_bytes, stream, nullptr);
}
extern "C" int tmi_lm_head_sample(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                  float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                  float temperature, int64_t top_k, float top_p, uint64_t seed, int32_t suppress_id,
                                  int32_t eos_id, int32_t pad_id, int32_t* finished, int32_t* ids, int64_t ids_ld,
                                  float* logprob, int32_t* n_finished, void* workspace, int64_t workspace_bytes,
                                  void* stream) {
  return tmi_plan_run<tmi_lm_head_sample_impl>(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, temperature,
                                               top_k, top_p, seed, suppress_id, eos_id, pad_id, finished, ids, ids_ld,
                                               logprob, n_finished, workspace, workspace_bytes, stream);
}
static int tmi_lm_head_sample_c_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                     float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                     float temperature, int64_t top_k, float top_p, uint64_t seed, int32_t suppress_id,
                                     int32_t eos_id, int32_t pad_id, int32_t* finished, int32_t* ids, int64_t ids_ld,
                                     float* logprob, int32_t* n_finished, void* workspace, int64_t workspace_bytes,
                                     const uint32_t* seen, const uint32_t* banned, int64_t bits_ld, float penalty,
                                     void* stream) {
  am_cons c;
  const am_cons* cs;
  if (!am_cons_args(seen, banned, bits_ld, penalty, V, c, cs)) {
    tmi_set_error("tmi_lm_head_sample_c: bad argument");
    return TMI_ERR_INVALID;
  }
  return sm_run("tmi_lm_head_sample_c: bad argument", x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V,
                temperature, top_k, top_p, seed, suppress_id, eos_id, pad_id, finished, ids, ids_ld, logprob, n_finished,
                workspace, workspace_bytes, stream, cs);
}
extern "C" int tmi_lm_head_sample_c(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                    float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                    float temperature, int64_t top_k, float top_p, uint64_t seed, int32_t suppress_id,
                                    int32_t eos_id, int32_t pad_id, int32_t* finished, int32_t* ids, int64_t ids_ld,
                                    float* logprob, int32_t* n_finished, void* workspace, int64_t workspace_bytes,
                                    const uint32_t* seen, const uint32_t* banned, int64_t bits_ld, float penalty,
                                    void* stream) {
  return tmi_plan_run<tmi_lm_head_sample_c_impl>(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, temperature,
                                                 top_k, top_p, seed, suppress_id, eos_id, pad_id, finished, ids, ids_ld,
                                                 logprob, n_finished, workspace, workspace_bytes, seen, banned, bits_ld,
                                                 penalty, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// tmi_decode_constraints: the two bit sets of the _c LM heads for M rows, from the rows' current prefixes; the rule is
// include/tethys_mi.h's.  One workgroup per row, both sets built in LDS (8 KiB each at V = 65536) with LDS atomic ORs - an
// OR does not depend on the order, so the words are the same in every run - and written out once, every one of the W
// words: the caller never clears them.  The work is a few hundred loads; the cost is the launch.
namespace {
constexpr int CN_THREADS = 256;
constexpr int CN_MAXV = 65536;

__global__ __launch_bounds__(CN_THREADS) void decode_constraints_kernel(
    const int32_t* __restrict__ prefix, int64_t ld, int t, int V, int W, const uint32_t* __restrict__ static_banned, int ngram,
    uint32_t* __restrict__ seen, uint32_t* __restrict__ banned, int64_t bits_ld) {
  __shared__ uint32_t s_seen[CN_MAXV / 32], s_ban[CN_MAXV / 32];
  const int tid = threadIdx.x;
  const int32_t* p = prefix + (int64_t)blockIdx.x * ld;
  for (int i = tid; i < W; i += CN_THREADS) {
    s_seen[i] = 0;
    s_ban[i] = static_banned ? static_banned[i] : 0;
  }
  __syncthreads();
  for (int j = tid; j < t; j += CN_THREADS) {
    const uint32_t x = (uint32_t)p[j];
    if (x < (uint32_t)V) atomicOr(&s_seen[x >> 5], 1u << (x & 31));  // (an id outside [0, V) sets no bit)
  }
  const int g = ngram - 1;  // the length of the context: the last g tokens of the prefix
  if (ngram >= 1 && g <= t) {
    for (int j = tid; j + g < t; j += CN_THREADS) {  // (the token after the match is column j + g <= t - 1)
      bool same = true;
      for (int i = 0; i < g && same; ++i) same = p[j + i] == p[t - g + i];
      const uint32_t x = (uint32_t)p[j + g];
      if (same && x < (uint32_t)V) atomicOr(&s_ban[x >> 5], 1u << (x & 31));
    }
  }
  __syncthreads();
  const uint32_t last = (V & 31) ? ((1u << (V & 31)) - 1u) : 0xffffffffu;  // bits at or above V stay 0
  for (int i = tid; i < W; i += CN_THREADS) {
    const uint32_t mask = i == W - 1 ? last : 0xffffffffu;
    seen[(int64_t)blockIdx.x * bits_ld + i] = s_seen[i] & mask;
    banned[(int64_t)blockIdx.x * bits_ld + i] = s_ban[i] & mask;
  }
}
}  // namespace

static int tmi_decode_constraints_impl(const int32_t* prefix, int64_t ld, int64_t M, int64_t t, int64_t V,
                                       const uint32_t* static_banned, int64_t ngram, uint32_t* seen, uint32_t* banned,
                                       int64_t bits_ld, void* stream) {
  const int64_t W = (V + 31) / 32;
  if (!prefix || !seen || !banned || M < 1 || M > 65535 || V < 1 || V > CN_MAXV || t < 1 || t > 65536 || t > ld || ngram < 0 ||
      ngram > INT32_MAX || bits_ld < W) {
    tmi_set_error("tmi_decode_constraints: bad argument");
    return TMI_ERR_INVALID;
  }
  hipLaunchKernelGGL(decode_constraints_kernel, dim3((unsigned)M), dim3(CN_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     prefix, ld, (int)t, (int)V, (int)W, static_banned, (int)ngram, seen, banned, bits_ld);
  return tmi_check_launch("tmi_decode_constraints");
}
extern "C" int tmi_decode_constraints(const int32_t* prefix, int64_t ld, int64_t M, int64_t t, int64_t V,
                                      const uint32_t* static_banned, int64_t ngram, uint32_t* seen, uint32_t* banned,
                                      int64_t bits_ld, void* stream) {
  return tmi_plan_run<tmi_decode_constraints_impl>(prefix, ld, M, t, V, static_banned, ngram, seen, banned, bits_ld, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Whisper's timestamp-token grammar; the rules are include/tethys_mi.h's "Timestamp rules" (a - g).
//
// tmi_timestamp_rules: rules a - f, one workgroup per row.  The row's state (n, last, pen, tl) comes from one scan of the
// generated tokens (the last timestamp by a max over positions: wave shuffles, then the four waves through LDS); every ban
// of a - f is then one of at most three column ranges - the below columns [0, tb) less EOS, the timestamps [tb, lo_hi) and
// the timestamps [hi_lo, V) - plus the one no-timestamps bit, so a thread ORs the ranges' share of a word into the word it
// owns with a plain load and store.  A word with nothing to add is not written.
namespace {
__device__ __forceinline__ uint32_t ts_range_word(int i, int lo, int hi) {  // bits of [lo, hi) in word i
  const int a = max(lo, 32 * i) - 32 * i, b = min(hi, 32 * i + 32) - 32 * i;
  if (a >= b) return 0u;
  return (b == 32 ? 0xffffffffu : (1u << b) - 1u) & ~((1u << a) - 1u);
}

__global__ __launch_bounds__(CN_THREADS) void timestamp_rules_kernel(
    const int32_t* __restrict__ prefix, int64_t ld, int t, int P, int V, int W, int tb, int no_ts, int eos, int max_initial,
    int max_ts, uint32_t* __restrict__ banned, int64_t bits_ld) {
  __shared__ int s_best[CN_THREADS / 64];
  const int tid = threadIdx.x;
  const int32_t* g = prefix + (int64_t)blockIdx.x * ld + 1 + P;
  const int n = t - 1 - P;
  auto is_ts = [&](int32_t x) { return x >= tb && x < V; };  // (an id outside [0, V) is no timestamp: never an index)
  int best = -1;
  for (int j = tid; j < n; j += CN_THREADS)
    if (is_ts(g[j])) best = j;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
  if ((tid & 63) == 0) s_best[tid >> 6] = best;
  __syncthreads();
  best = max(max(s_best[0], s_best[1]), max(s_best[2], s_best[3]));
  const bool last = n >= 1 && is_ts(g[n - 1]);
  const bool pen = n < 2 || is_ts(g[n - 2]);
  const bool closed = last && !pen;  // a closing timestamp: rules d and e
  // the below columns [0, below_hi), less EOS when a closing timestamp precedes (b, d)
  const int below_hi = (n == 0 || closed) ? tb : 0;
  const int keep = closed ? eos : -1;
  // the timestamps [tb, lo_hi) (c, e, f) and [hi_lo, V) (a, b)
  int lo_hi = tb;
  if (best >= 0) lo_hi = closed ? g[best] : g[best] + 1;
  if (last && pen) lo_hi = V;
  int hi_lo = tb + max_ts + 1;
  if (n == 0 && max_initial >= 0) hi_lo = min(hi_lo, tb + max_initial + 1);
  uint32_t* row = banned + (int64_t)blockIdx.x * bits_ld;
  for (int i = tid; i < W; i += CN_THREADS) {
    uint32_t m = ts_range_word(i, 0, below_hi);
    if (keep >= 0 && (keep >> 5) == i && keep < below_hi) m &= ~(1u << (keep & 31));
    m |= ts_range_word(i, tb, min(lo_hi, V)) | ts_range_word(i, min(hi_lo, V), V);
    if (no_ts >= 0 && (no_ts >> 5) == i) m |= 1u << (no_ts & 31);
    if (m) row[i] |= m;
  }
}
}  // namespace

static int tmi_timestamp_rules_impl(const int32_t* prefix, int64_t ld, int64_t M, int64_t t, int64_t P, int64_t V, int64_t tb,
                                    int32_t no_timestamps_id, int32_t eos_id, int64_t max_initial, int64_t max_ts,
                                    uint32_t* banned, int64_t bits_ld, void* stream) {
  const int64_t W = (V + 31) / 32;
  if (!prefix || !banned || (reinterpret_cast<uintptr_t>(banned) & 3) || M < 1 || M > 65535 || V < 1 || V > CN_MAXV || t < 1 ||
      t > 65536 || t > ld || P < 0 || 1 + P > t || tb < 0 || tb > V || no_timestamps_id >= V || eos_id >= V || max_ts < 0 ||
      bits_ld < W) {
    tmi_set_error("tmi_timestamp_rules: bad argument");
    return TMI_ERR_INVALID;
  }
  const int no_ts = no_timestamps_id < 0 ? -1 : no_timestamps_id, eos = eos_id < 0 ? -1 : eos_id;
  const int mi = max_initial < 0 ? -1 : (int)(max_initial < V ? max_initial : V);  // (a cap at or past V bans nothing)
  const int mt = (int)(max_ts < V ? max_ts : V);
  hipLaunchKernelGGL(timestamp_rules_kernel, dim3((unsigned)M), dim3(CN_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     prefix, ld, (int)t, (int)P, (int)V, (int)W, (int)tb, no_ts, eos, mi, mt, banned, bits_ld);
  return tmi_check_launch("tmi_timestamp_rules");
}
extern "C" int tmi_timestamp_rules(const int32_t* prefix, int64_t ld, int64_t M, int64_t t, int64_t P, int64_t V, int64_t tb,
                                   int32_t no_timestamps_id, int32_t eos_id, int64_t max_initial, int64_t max_ts,
                                   uint32_t* banned, int64_t bits_ld, void* stream) {
  return tmi_plan_run<tmi_timestamp_rules_impl>(prefix, ld, M, t, P, V, tb, no_timestamps_id, eos_id, max_initial, max_ts,
                                                banned, bits_ld, stream);
}

// tmi_lm_head_timestamp_gate: rule g.  The LM-head body of the kernels above (am_head_tile) and their z' (am_cons_bits,
// am_cons_logit), with a reduction as the epilogue: per workgroup and row the max of z' over its below columns and the
// (max, sum exp) pair over its timestamp columns, banned columns left out of both (16 lanes of 8 columns, a fixed butterfly),
// stored in the row's slot for this workgroup - a plain 16-byte store.  The last workgroup of a row tile (one completion
// counter per tile, the top-k kernel's pattern) works one wave per row: lane w folds slots w, w + 64, .. in order, a
// butterfly that pairs the lower lane first finishes the logsumexp, so the bits do not depend on the arrival order; it
// writes fired[r], puts the slots back to zero and - only now, when every workgroup that reads the row's banned words has
// delivered its partial - ORs the below columns into banned[r] where the rule fired.
namespace {
// grid (ceil(V / 128), ceil(M / MT)); dynamic LDS max(d * MT, 4 * MT * 128) floats
template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_timestamp_gate_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, const uint32_t* seen, uint32_t* banned,
    int64_t bits_ld, float penalty, int tb, int32_t* __restrict__ fired, uint32_t* __restrict__ counters,
    f32x4* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) float am_lds[];
  __shared__ int tg_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * MT;
  const int rows = min(MT, M - row0);
  const int nwg = gridDim.x;
  am_head_tile<TW, MT>(am_lds, xv, x_ld, x_bf16, gamma, beta, eps, w, w_ld, d, V, row0, rows);
  const float* red = am_lds;
  const am_cons cs{seen, banned, bits_ld, penalty};

  // ---- per row (16 lanes of 8 columns): max z' below tb, (max, sum exp) of z' from tb up
  {
    const int m = tid >> 4, g = tid & 15;
    if (m < rows) {
      const int r = row0 + m;
      const int c0 = blockIdx.x * AM_COLS + g * 8;
      uint32_t sb, bb;
      am_cons_bits<true>(cs, r, c0, V, sb, bb);
      float v[8];
      float mb = -INFINITY, mt = -INFINITY;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int o = m * AM_COLS + g * 8 + c;
        const float z = ((red[o] + red[MT * AM_COLS + o]) + red[2 * MT * AM_COLS + o]) + red[3 * MT * AM_COLS + o];
        v[c] = am_cons_logit<true>(z, sb, bb, c, cs.penalty);
        const bool ok = c0 + c < V && !((bb >> c) & 1u);
        if (ok && c0 + c < tb) mb = fmaxf(mb, v[c]);
        if (ok && c0 + c >= tb) mt = fmaxf(mt, v[c]);
      }
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        mb = fmaxf(mb, __shfl_xor(mb, o, 64));
        mt = fmaxf(mt, __shfl_xor(mt, o, 64));
      }
      float se = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        se += (c0 + c < V && c0 + c >= tb && !((bb >> c) & 1u) && mt > -INFINITY) ? expf(v[c] - mt) : 0.f;
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) se += __shfl_xor(se, o, 64);  // (xor pairs: both lanes add the same two values)
      if (g == 0) part[(int64_t)r * nwg + blockIdx.x] = f32x4{mb, mt, se, 0.f};
    }
  }

  // ---- completion: the last workgroup of the row tile folds, publishes and cleans up
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(counters + blockIdx.y, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    tg_last = prev == (uint32_t)nwg - 1;
  }
  __syncthreads();
  if (!tg_last) return;
  __threadfence();
  for (int m = wave; m < rows; m += 4) {
    const int r = row0 + m;
    float below = -INFINITY, am = -INFINITY, as = 0.f;
    f32x4* slot = part + (int64_t)r * nwg;
    f32x4 pv[TK_HEADS];  // (ceil(V / 128) <= 512 slots: at most 8 a lane, all loads in flight before the first fold)
#pragma unroll
    for (int i = 0; i < TK_HEADS; ++i) {
      const int wg = lane + 64 * i;
      pv[i] = wg < nwg ? slot[wg] : f32x4{-INFINITY, -INFINITY, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < TK_HEADS; ++i) {
      below = fmaxf(below, pv[i][0]);
      lse_fold(am, as, pv[i][1], pv[i][2]);
      if (lane + 64 * i < nwg) slot[lane + 64 * i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      below = fmaxf(below, __shfl_xor(below, o, 64));
      const float om = __shfl_xor(am, o, 64), os = __shfl_xor(as, o, 64);
      if (lane & o) {  // the lower lane's pair first, in both lanes
        float lm = om, ls = os;
        lse_fold(lm, ls, am, as);
        am = lm, as = ls;
      } else {
        lse_fold(am, as, om, os);
      }
    }
    const float lse = am == -INFINITY ? -INFINITY : am + logf(as);
    const bool fire = lse > below;  // (strict, fp32; -inf on both sides does not fire)
    if (lane == 0) fired[r] = fire ? 1 : 0;
    if (fire) {
      uint32_t* row = banned + (int64_t)r * bits_ld;
      const int full = tb >> 5;
      for (int i = lane; i < full; i += 64) row[i] = 0xffffffffu;
      if (lane == 0 && (tb & 31)) row[full] |= (1u << (tb & 31)) - 1u;
    }
  }
  __syncthreads();
  if (tid == 0) __hip_atomic_store(counters + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
}  // namespace

extern "C" int64_t tmi_lm_head_timestamp_gate_workspace_bytes(int64_t M, int64_t V) {
  if (M < 1 || V < 1 || V > CN_MAXV) return -1;
  return 16 * M * (1 + (V + AM_COLS - 1) / AM_COLS);
}

static int tmi_lm_head_timestamp_gate_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                           float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d,
                                           int64_t V, const uint32_t* seen, uint32_t* banned, int64_t bits_ld, float penalty,
                                           int64_t tb, int32_t* fired, void* workspace, int64_t workspace_bytes, void* stream) {
  am_geom g;
  const bool shared_ok = am_args(x, x_ld, x_dtype, gamma, beta, w, w_ld, w_dtype, M, d, V, workspace, g);
  if (!shared_ok || !banned || !fired || V > CN_MAXV || tb < 0 || tb > V || !(penalty > 0.f && penalty < INFINITY) ||
      bits_ld < (V + 31) / 32 || ((reinterpret_cast<uintptr_t>(seen) | reinterpret_cast<uintptr_t>(banned)) & 3) ||
      !tmi_aligned(workspace, 16) || workspace_bytes < tmi_lm_head_timestamp_gate_workspace_bytes(M, V)) {
    tmi_set_error("tmi_lm_head_timestamp_gate: bad argument");
    return TMI_ERR_INVALID;
  }
  char* base = reinterpret_cast<char*>(workspace);
  uint32_t* counters = reinterpret_cast<uint32_t*>(base);  // (one per row tile; 16 * M bytes reserved)
  f32x4* part = reinterpret_cast<f32x4*>(base + 16 * M);
  const int xb = x_dtype == TMI_BF16;
  const dim3 grid((unsigned)g.nwg, (unsigned)((M + g.MT - 1) / g.MT));
  return am_dispatch(w_dtype, g.MT, [&](auto tw, auto mt) {
    using TW = typename decltype(tw)::type;
    return am_launch_one<lm_head_timestamp_gate_kernel<TW, mt()>>(
        "tmi_lm_head_timestamp_gate", grid, (size_t)g.lds_floats * 4, reinterpret_cast<hipStream_t>(stream), x, x_ld, xb, gamma,
        beta, eps, reinterpret_cast<const TW*>(w), w_ld, (int)M, (int)d, (int)V, seen, banned, bits_ld, penalty, (int)tb, fired,
        counters, part);
  });
}
extern "C" int tmi_lm_head_timestamp_gate(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                          float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d,
                                          int64_t V, const uint32_t* seen, uint32_t* banned, int64_t bits_ld, float penalty,
                                          int64_t tb, int32_t* fired, void* workspace, int64_t workspace_bytes, void* stream) {
  return tmi_plan_run<tmi_lm_head_timestamp_gate_impl>(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, seen,
                                                       banned, bits_ld, penalty, tb, fired, workspace, workspace_bytes, stream);
}
