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

namespace {

constexpr int AM_THREADS = 256;
constexpr int AM_COLS = 128;      // columns per workgroup: 16 column groups of 8
constexpr int AM_KSLICES = 16;    // row slices per workgroup

// order-preserving map of an fp32 value onto uint32 (-0 folded onto +0 first: tf.argmax sees them equal)
__device__ __forceinline__ uint32_t am_order(float v) {
  const uint32_t u = __float_as_uint(v + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
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

// grid (ceil(V / 128), ceil(M / MT)); dynamic LDS max(d * MT, 4 * MT * 128) floats
template <typename TW, int MT>
__global__ __launch_bounds__(AM_THREADS) void lm_head_argmax_kernel(
    const void* __restrict__ xv, int64_t x_ld, int x_bf16, const float* __restrict__ gamma, const float* __restrict__ beta,
    float eps, const TW* __restrict__ w, int64_t w_ld, int M, int d, int V, int32_t* __restrict__ ids, int64_t ids_ld,
    int eos_id, int32_t* __restrict__ eos_count, uint64_t* __restrict__ slots, uint32_t* __restrict__ counter) {
  extern __shared__ __attribute__((aligned(16))) float am_lds[];
  __shared__ int am_last, am_eos;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int row0 = blockIdx.y * MT;
  const int rows = min(MT, M - row0);

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

  // ---- per row: best key over the workgroup's 128 columns (16 lanes of 8 columns), one atomic max per row
  {
    const int m = tid >> 4, g = tid & 15;
    uint64_t best = 0;  // 0 = no candidate (every real key is larger: its ~column half is nonzero or its value half is)
    if (m < rows) {
      const int c0 = blockIdx.x * AM_COLS + g * 8;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int col = c0 + c;
        const int o = m * AM_COLS + g * 8 + c;
        const float v = ((red[o] + red[MT * AM_COLS + o]) + red[2 * MT * AM_COLS + o]) + red[3 * MT * AM_COLS + o];
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
int am_launch(dim3 grid, size_t lds, hipStream_t s, const void* x, int64_t x_ld, int x_bf16, const float* gamma,
              const float* beta, float eps, const void* w, int64_t w_ld, int M, int d, int V, int32_t* ids, int64_t ids_ld,
              int eos_id, int32_t* eos_count, uint64_t* slots, uint32_t* counter) {
  auto kern = lm_head_argmax_kernel<TW, MT>;
  // above 64 KiB of dynamic LDS (16 rows of d > 1024) the kernel has to opt in, up to what it needs (160 KiB per CU on
  // gfx950, its few static bytes included)
  static size_t opted = 65536;
  if (lds > opted) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
        hipSuccess) {
      (void)hipGetLastError();
      tmi_set_error("tmi_lm_head_argmax: the LDS size could not be granted");
      return TMI_ERR_LAUNCH;
    }
    opted = lds;
  }
  hipLaunchKernelGGL(kern, grid, dim3(AM_THREADS), lds, s, x, x_ld, x_bf16, gamma, beta, eps,
                     reinterpret_cast<const TW*>(w), w_ld, M, d, V, ids, ids_ld, eos_id, eos_count, slots, counter);
  return tmi_check_launch("tmi_lm_head_argmax");
}

template <typename TW>
int am_dispatch(int MT, dim3 grid, size_t lds, hipStream_t s, const void* x, int64_t x_ld, int x_bf16, const float* gamma,
                const float* beta, float eps, const void* w, int64_t w_ld, int M, int d, int V, int32_t* ids,
                int64_t ids_ld, int eos_id, int32_t* eos_count, uint64_t* slots, uint32_t* counter) {
#define AM_CASE(n)                                                                                                  \
  case n:                                                                                                           \
    return am_launch<TW, n>(grid, lds, s, x, x_ld, x_bf16, gamma, beta, eps, w, w_ld, M, d, V, ids, ids_ld, eos_id, \
                            eos_count, slots, counter);
  switch (MT) {
    AM_CASE(1) AM_CASE(2) AM_CASE(4) AM_CASE(8) AM_CASE(16)
  }
#undef AM_CASE
  return TMI_ERR_INVALID;
}

inline bool am_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

static int tmi_lm_head_argmax_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                   float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                   int32_t* ids, int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace,
                                   int64_t workspace_bytes, void* stream);
extern "C" int tmi_lm_head_argmax(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                  float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                  int32_t* ids, int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  if (tmi_plan_recording())
    tmi_plan_push([=]() -> int {
      return tmi_lm_head_argmax(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, ids, ids_ld, eos_id, eos_count,
                                workspace, workspace_bytes, stream);
    });
  tmi_plan_enter();
  const int rc_ = tmi_lm_head_argmax_impl(x, x_ld, x_dtype, gamma, beta, eps, w, w_ld, w_dtype, M, d, V, ids, ids_ld, eos_id,
                                          eos_count, workspace, workspace_bytes, stream);
  tmi_plan_leave();
  return rc_;
}
static int tmi_lm_head_argmax_impl(const void* x, int64_t x_ld, int32_t x_dtype, const float* gamma, const float* beta,
                                   float eps, const void* w, int64_t w_ld, int32_t w_dtype, int64_t M, int64_t d, int64_t V,
                                   int32_t* ids, int64_t ids_ld, int32_t eos_id, int32_t* eos_count, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  const bool dt_ok = (x_dtype == TMI_F32 || x_dtype == TMI_BF16) && (w_dtype == TMI_F32 || w_dtype == TMI_BF16);
  const int MT = M <= 1 ? 1 : M <= 2 ? 2 : M <= 4 ? 4 : M <= 8 ? 8 : 16;
  const int64_t lds_floats = d * MT > 4 * MT * AM_COLS ? d * MT : 4 * MT * AM_COLS;
  if (!x || !w || !ids || !workspace || !dt_ok || M < 1 || M > (int64_t)16 * 65535 || d < 1 || V < 1 || V >= INT32_MAX ||
      w_ld < V || (w_ld & 7) || !am_al16(w) || x_ld < d || ids_ld < 1 || (gamma == nullptr) != (beta == nullptr) ||
      workspace_bytes < 8 * (M + 1) || (reinterpret_cast<uintptr_t>(workspace) & 7) || lds_floats * 4 > 160 * 1024 - 256) {
    tmi_set_error("tmi_lm_head_argmax: bad argument");
    return TMI_ERR_INVALID;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  uint64_t* slots = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* counter = reinterpret_cast<uint32_t*>(slots + M);
  const dim3 grid((unsigned)((V + AM_COLS - 1) / AM_COLS), (unsigned)((M + MT - 1) / MT));
  const size_t lds = (size_t)lds_floats * 4;
  const int xb = x_dtype == TMI_BF16;
  if (w_dtype == TMI_BF16)
    return am_dispatch<bf16_t>(MT, grid, lds, s, x, x_ld, xb, gamma, beta, eps, w, w_ld, (int)M, (int)d, (int)V, ids, ids_ld,
                               eos_id, eos_count, slots, counter);
  return am_dispatch<float>(MT, grid, lds, s, x, x_ld, xb, gamma, beta, eps, w, w_ld, (int)M, (int)d, (int)V, ids, ids_ld,
                            eos_id, eos_count, slots, counter);
}
