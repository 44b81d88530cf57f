// The learned weighted sum over encoder layers in front of the CTC head (the frozen-encoder probe of SUPERB / s3prl,
// `use_weighted_layer_sum`): tmi_layer_mix_fwd, tmi_layer_mix_bwd, tmi_layer_mix_workspace_bytes.  include/tethys_mi.h states
// the contract; this is how it is carried out.  All arithmetic is fp32, there is no atomic, and every floating-point sum runs
// in an order fixed by (N, T_max, H, V, K) alone, so the same call gives the same bits.  Rows, liveness, the gather through
// row_index and the clamping of device values are those of csrc/ctc_head.hip: row r = n * T_max + t is live when
// t < min(frame_lens[n], T_max); a dead row is never read and never written.
//
// The K layer pointers travel to the kernels BY VALUE in a struct (512 bytes of kernel arguments): the caller builds no
// device-side pointer table, and the layers may be separate allocations or slices of one stacked tensor.
//
// lm_softmax - every workgroup forms w = softmax(a) the same way: lane k < K of wave 0 holds a[k]; m = the maximum (exact in
//   any order), e_k = expf(a[k] - m) goes to LDS, then every lane adds e_0 + e_1 + .. in ascending k from e_0 and divides.
// layer_mix_fwd_kernel - one thread per 8 consecutive columns of one row (a 16-byte load of bf16, two of fp32), 256 threads a
//   workgroup, rows * H / 8 threads in all (750 workgroups at 2000 rows of 768).  The layers are read LM_LB = 8 at a time:
//   the 8 loads are issued before the first of their fused multiply-adds, acc = fmaf(w_k, x_k, acc) for k ascending.
// layer_mix_bwd_kernel - one workgroup per tile of `tr` consecutive rows, tr = 8 * ceil(N * T_max / 8192): at most 1024 tiles
//   (249 at N 8 / T 249), so the workspace stays at 1024 K floats.  H is walked in slices of hs = 256 columns (128 when
//   V > 32); the slice of W goes to LDS transposed, Wt[v][h], so that a thread reads its 8 columns of one v as two 16-byte
//   LDS loads.  A slice is covered by hs / 8 threads per row, so 256 / (hs / 8) = 8 (16) rows are in flight at a time: per
//   pass their gs = grad * w_n go to LDS, a thread forms dx of its 8 columns (fmaf over v ascending from 0), applies the
//   dropout mask of the head's forward (tmi_drop8: position r, column h), and adds dx[i] * x_k[i], i = 0 .. 7 ascending, into
//   its accumulator of layer k (fmaf), the layers again 8 loads at a time.  A thread's chain runs over the slices in
//   ascending order, inside a slice over its rows ascending.  Then the 64 lanes of a wave meet in the xor butterfly 32, 16,
//   .., 1, the four waves are added ((w0 + w1) + w2) + w3, and part[tile][k] is stored.
// layer_mix_fold_kernel - one workgroup; wave w takes the layers w, w + 4, ..: lane l adds the tiles l, l + 64, .. ascending
//   from 0, the lanes meet in the same butterfly: d_k.  Then g_a[k] = w_k * (d_k - sum_j w_j d_j), the inner sum a chain of
//   fmaf over j ascending from 0.
// SpecAugment (tmi_layer_mix_bwd_m; the bits of tmi_spec_masks): the backward kernel is a template on MASKED, and the existing
//   entry point launches the instantiation without it.  With it a time-masked row is skipped like a dead one, and dx is
//   zeroed under the byte of the feature word that covers the thread's 8 columns, right after the dropout mask.
#include "tmi_common.h"
#include <math.h>

namespace {

constexpr int LM_THREADS = 256;
constexpr int LM_MAXK = 64;
constexpr int LM_LB = 8;             // layers whose loads are in flight together
constexpr int LM_TR = 8;             // backward: the row tile is a multiple of this
constexpr int LM_MAXTILES = 1024;    // backward: tiles at most
constexpr int LM_WT = 8448;          // backward: floats of the transposed W slice (32 x 260 or 64 x 132, rows padded by 4)
constexpr int64_t LM_MAXN = 65535, LM_MAXT = 4096, LM_MAXROWS = (int64_t)1 << 22, LM_MAXH = 4096, LM_MAXV = 64, LM_MAXL = 511;

struct layers_t {
  const void* p[LM_MAXK];
};

struct rows_t {  // what locates a row: as in ctc_head.hip
  int64_t x_sn, x_st, n_src;
  const int32_t* row_index;
  const int32_t* frame_lens;
  int N, T_max;
  bool vec;  // 16-byte loads of 8 elements are aligned
};

__device__ __forceinline__ int lm_frames(const rows_t& g, int n) {
  const int f = g.frame_lens[n];
  return f < 0 ? 0 : (f > g.T_max ? g.T_max : f);
}
__device__ __forceinline__ int64_t lm_src(const rows_t& g, int n) {
  const int64_t s = g.row_index ? (int64_t)g.row_index[n] : (int64_t)n;
  return (s >= 0 && s < g.n_src) ? s : -1;
}

// what one 8-element load returns, kept raw so that LM_LB of them can be in flight before any is converted
template <typename T> struct raw8;
template <> struct raw8<bf16_t> {
  bf16x8 q;
};
template <> struct raw8<float> {
  f32x4 a, b;
};

template <typename T>
__device__ __forceinline__ raw8<T> lm_load8(const void* layer, int64_t off, bool vec) {
  const T* __restrict__ p = reinterpret_cast<const T*>(layer) + off;
  raw8<T> r;
  if constexpr (sizeof(T) == 2) {
    if (vec) {
      r.q = *reinterpret_cast<const bf16x8*>(p);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) r.q[i] = p[i];
    }
  } else {
    if (vec) {
      r.a = *reinterpret_cast<const f32x4*>(p), r.b = *reinterpret_cast<const f32x4*>(p + 4);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) r.a[i] = p[i], r.b[i] = p[4 + i];
    }
  }
  return r;
}
__device__ __forceinline__ float lm_at(const raw8<bf16_t>& r, int i) { return (float)r.q[i]; }
__device__ __forceinline__ float lm_at(const raw8<float>& r, int i) { return i < 4 ? r.a[i] : r.b[i - 4]; }

// w = softmax(a) into ws[0 .. K): called by every thread of a workgroup of >= 64 threads; es, ws: LM_MAXK floats of LDS each
__device__ __forceinline__ void lm_softmax(const float* __restrict__ a, int K, float* es, float* ws) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const float v = tid < K ? a[tid] : -INFINITY;
    const float m = wave_max(v);
    if (tid < K) es[tid] = expf(v - m);
  }
  __syncthreads();
  if (tid < K) {
    float s = es[0];
    for (int k = 1; k < K; ++k) s += es[k];
    ws[tid] = es[tid] / s;
  }
  __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(LM_THREADS) void layer_mix_fwd_kernel(layers_t L, int K, rows_t g, const float* __restrict__ a,
                                                                  float* __restrict__ w_out, float* __restrict__ mixed,
                                                                  int64_t m_sn, int64_t m_st, bool m_vec, int H) {
  __shared__ float es[LM_MAXK], ws[LM_MAXK];
  lm_softmax(a, K, es, ws);
  if (blockIdx.x == 0 && w_out != nullptr && threadIdx.x < K) w_out[threadIdx.x] = ws[threadIdx.x];
  const int H8 = H >> 3;
  const int64_t e = (int64_t)blockIdx.x * LM_THREADS + threadIdx.x;
  const int64_t r = e / H8;
  if (r >= (int64_t)g.N * g.T_max) return;
  const int c = (int)(e - r * H8) * 8;
  const int n = (int)(r / g.T_max), t = (int)(r - (int64_t)n * g.T_max);
  if (t >= lm_frames(g, n)) return;
  const int64_t s = lm_src(g, n);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (s >= 0) {
    const int64_t off = s * g.x_sn + (int64_t)t * g.x_st + c;
    for (int kb = 0; kb < K; kb += LM_LB) {
      raw8<T> q[LM_LB];
#pragma unroll
      for (int j = 0; j < LM_LB; ++j)
        if (kb + j < K) q[j] = lm_load8<T>(L.p[kb + j], off, g.vec);
#pragma unroll
      for (int j = 0; j < LM_LB; ++j)
        if (kb + j < K) {
          const float w = ws[kb + j];
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i] = fmaf(w, lm_at(q[j], i), acc[i]);
        }
    }
  }
  float* __restrict__ o = mixed + (int64_t)n * m_sn + (int64_t)t * m_st + c;
  if (m_vec) {
    *reinterpret_cast<f32x4*>(o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    *reinterpret_cast<f32x4*>(o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = acc[i];
  }
}

// w_n of a feasible item, as ctc_head.hip forms it: 1 ("sum") or 1 / (max(L, 1) * N) ("mean"), L clamped to [0, L_max]
__device__ __forceinline__ float lm_weight(const int32_t* __restrict__ label_lens, int n, int N, int L_max, int reduction) {
  if (reduction == 0) return 1.0f;
  int L = label_lens[n];
  L = L < 1 ? 1 : (L > L_max ? L_max : L);
  return 1.0f / ((float)L * (float)N);
}

struct drop_t {
  uint32_t key, thr;
  float scale;
  bool on;
};

struct mask_t {  // span masks by position n (tmi_spec_masks' layout); a NULL pointer: that mask is off
  const uint32_t* time_bits;
  const uint32_t* feat_bits;
  int64_t ld_t, ld_f;
};

template <typename T, int KM, bool MASKED>
__global__ __launch_bounds__(LM_THREADS) void layer_mix_bwd_kernel(layers_t L, int K, rows_t g,
                                                                  const int32_t* __restrict__ label_lens,
                                                                  const float* __restrict__ grad, int64_t gr_sn, int64_t gr_st,
                                                                  const int32_t* __restrict__ infeasible, drop_t drop,
                                                                  int reduction, const float* __restrict__ W,
                                                                  float* __restrict__ part, int L_max, int H, int V, int tr,
                                                                  mask_t mk) {
  __shared__ __attribute__((aligned(16))) float Wt[LM_WT];
  __shared__ float gss[16 * LM_MAXV];
  __shared__ float red[4][KM];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int hs = V <= 32 ? 256 : 128, hsp = hs + 4;  // columns per slice, and the padded row of Wt
  const int tpr = hs >> 3, rp = LM_THREADS / tpr;    // threads per row, rows per pass
  const int slot = tid / tpr, c = (tid - slot * tpr) * 8;
  const int R = g.N * g.T_max;
  const int row_lo = blockIdx.x * tr, row_hi = row_lo + tr < R ? row_lo + tr : R;
  float acc[KM];
#pragma unroll
  for (int k = 0; k < KM; ++k) acc[k] = 0.f;
  for (int h0 = 0; h0 < H; h0 += hs) {
    const int hl = H - h0 < hs ? H - h0 : hs;  // (a multiple of 8)
    __syncthreads();
    for (int e = tid; e < hl * V; e += LM_THREADS) {  // W[h0 + hh][v], contiguous from row h0 -> Wt[v][hh]
      const int hh = e / V, v = e - hh * V;
      Wt[v * hsp + hh] = W[(int64_t)h0 * V + e];
    }
    for (int rb = row_lo; rb < row_hi; rb += rp) {
      __syncthreads();
      for (int e = tid; e < rp * V; e += LM_THREADS) {  // gs of the pass's rows (zeros: dead, infeasible, past the tile)
        const int j = e / V, v = e - j * V, r = rb + j;
        float x = 0.f;
        if (r < row_hi) {
          const int n = r / g.T_max, t = r - n * g.T_max;
          if (t < lm_frames(g, n) && infeasible[n] == 0)
            x = grad[(int64_t)n * gr_sn + (int64_t)t * gr_st + v] * lm_weight(label_lens, n, g.N, L_max, reduction);
        }
        gss[e] = x;
      }
      __syncthreads();
      const int r = rb + slot;
      if (r >= row_hi || c >= hl) continue;  // (the barriers above are reached by every thread)
      const int n = r / g.T_max, t = r - n * g.T_max;
      if (t >= lm_frames(g, n) || infeasible[n] != 0) continue;
      const int64_t s = lm_src(g, n);
      if (s < 0) continue;  // every layer reads as zeros
      if constexpr (MASKED) {
        if (mk.time_bits != nullptr && ((mk.time_bits[(int64_t)n * mk.ld_t + (t >> 5)] >> (t & 31)) & 1u) != 0)
          continue;  // a time-masked row: `mixed` was zeros under the head, so dx meets zeros
      }
      float dx[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int v = 0; v < V; ++v) {
        const float gv = gss[slot * V + v];
        const f32x4 wa = *reinterpret_cast<const f32x4*>(&Wt[v * hsp + c]);
        const f32x4 wb = *reinterpret_cast<const f32x4*>(&Wt[v * hsp + c + 4]);
#pragma unroll
        for (int i = 0; i < 4; ++i) dx[i] = fmaf(gv, wa[i], dx[i]), dx[4 + i] = fmaf(gv, wb[i], dx[4 + i]);
      }
      if (drop.on) tmi_drop8(dx, r, h0 + c, drop.key, drop.thr, drop.scale);
      if constexpr (MASKED) {
        if (mk.feat_bits != nullptr) {  // the 8 columns are one byte of a word
          const uint32_t m = (mk.feat_bits[(int64_t)n * mk.ld_f + ((h0 + c) >> 5)] >> ((h0 + c) & 31)) & 0xffu;
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if ((m >> i) & 1u) dx[i] = 0.f;
        }
      }
      const int64_t off = s * g.x_sn + (int64_t)t * g.x_st + h0 + c;
#pragma unroll
      for (int kb = 0; kb < KM; kb += LM_LB) {
        if (kb >= K) break;
        raw8<T> q[LM_LB];
#pragma unroll
        for (int j = 0; j < LM_LB; ++j)
          if (kb + j < K) q[j] = lm_load8<T>(L.p[kb + j], off, g.vec);
#pragma unroll
        for (int j = 0; j < LM_LB; ++j)
          if (kb + j < K) {
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[kb + j] = fmaf(dx[i], lm_at(q[j], i), acc[kb + j]);
          }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < KM; ++k) {
    const float v = wave_sum(acc[k]);
    if (lane == 0) red[wv][k] = v;
  }
  __syncthreads();
  if (tid < K) part[(int64_t)blockIdx.x * K + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(LM_THREADS) void layer_mix_fold_kernel(const float* __restrict__ part, int ntiles, int K,
                                                                   const float* __restrict__ a, float* __restrict__ g_a,
                                                                   float* __restrict__ d_out) {
  __shared__ float es[LM_MAXK], ws[LM_MAXK], ds[LM_MAXK];
  lm_softmax(a, K, es, ws);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = wv; k < K; k += 4) {  // (uniform over the wave)
    float s = 0.f;
    for (int i = lane; i < ntiles; i += 64) s += part[(int64_t)i * K + k];
    s = wave_sum(s);
    if (lane == 0) ds[k] = s;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    float dot = 0.f;
    for (int j = 0; j < K; ++j) dot = fmaf(ws[j], ds[j], dot);
    g_a[threadIdx.x] = ws[threadIdx.x] * (ds[threadIdx.x] - dot);
    if (d_out != nullptr) d_out[threadIdx.x] = ds[threadIdx.x];
  }
}

bool lm_sizes_ok(int64_t N, int64_t T_max, int64_t H, int64_t K) {
  return N >= 1 && N <= LM_MAXN && T_max >= 1 && T_max <= LM_MAXT && N * T_max <= LM_MAXROWS && H >= 8 && H <= LM_MAXH &&
         H % 8 == 0 && K >= 1 && K <= LM_MAXK;
}
bool lm_v_ok(int64_t V) { return V >= 2 && V <= LM_MAXV; }
int64_t lm_tile_rows(int64_t R) { return LM_TR * ((R + (int64_t)LM_TR * LM_MAXTILES - 1) / ((int64_t)LM_TR * LM_MAXTILES)); }
int64_t lm_tiles(int64_t R) { return (R + lm_tile_rows(R) - 1) / lm_tile_rows(R); }
bool lm_p_ok(float p) { return p >= 0.f && p < 1.f && tmi_drop_ok(p); }
bool lm_stride_ok(int64_t sn, int64_t st, int64_t T_max, int64_t cols) {
  const int64_t lim = (int64_t)1 << 30;
  return st >= cols && st <= lim && sn >= T_max * st && sn <= lim;
}
inline bool f4(const void* p) { return p != nullptr && tmi_aligned(p, 4); }
inline bool f4n(const void* p) { return tmi_aligned(p, 4); }  // (may be NULL)
// K has been checked
bool lm_rows_ok(const layers_t& L, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index,
                const int32_t* frame_lens, int64_t N, int64_t T_max, int64_t H) {
  for (int64_t k = 0; k < K; ++k)
    if (L.p[k] == nullptr || !tmi_aligned(L.p[k], 16)) return false;
  return (x_dtype == TMI_F32 || x_dtype == TMI_BF16) && lm_stride_ok(x_sn, x_st, T_max, H) && n_src >= 1 &&
         n_src <= ((int64_t)1 << 30) && (row_index != nullptr || n_src >= N) && f4n(row_index) && f4(frame_lens);
}
rows_t lm_rows_of(int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index, const int32_t* frame_lens,
                  int64_t N, int64_t T_max) {
  rows_t g;
  g.x_sn = x_sn, g.x_st = x_st, g.n_src = n_src, g.row_index = row_index, g.frame_lens = frame_lens;
  g.N = (int)N, g.T_max = (int)T_max;
  const int64_t q = x_dtype == TMI_BF16 ? 8 : 4;  // elements per 16 bytes
  g.vec = x_sn % q == 0 && x_st % q == 0;
  return g;
}
// the host array, copied: a recorded launch plan keeps the pointers, not the caller's array
layers_t lm_layers_of(const void* const* layers, int64_t K) {
  layers_t L;
  for (int k = 0; k < LM_MAXK; ++k) L.p[k] = (layers != nullptr && k < K && K <= LM_MAXK) ? layers[k] : nullptr;
  return L;
}

}  // namespace

extern "C" int64_t tmi_layer_mix_workspace_bytes(int64_t N, int64_t T_max, int64_t H, int64_t V, int64_t K) {
  if (!lm_sizes_ok(N, T_max, H, K) || !lm_v_ok(V)) return -1;
  return lm_tiles(N * T_max) * K * 4;
}

static int tmi_layer_mix_fwd_impl(layers_t L, bool have_layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st,
                                  int64_t n_src, const int32_t* row_index, const int32_t* frame_lens, const float* a, float* w_out,
                                  float* mixed, int64_t m_sn, int64_t m_st, int64_t N, int64_t T_max, int64_t H, void* stream) {
  const bool ok = have_layers && lm_sizes_ok(N, T_max, H, K) &&
                  lm_rows_ok(L, K, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max, H) && f4(a) && f4n(w_out) &&
                  mixed != nullptr && tmi_aligned(mixed, 16) && lm_stride_ok(m_sn, m_st, T_max, H);
  if (!ok) {
    tmi_set_error("tmi_layer_mix_fwd: bad argument (1 <= K <= 64; 1 <= N <= 65535; 1 <= T_max <= 4096; N*T_max <= 2^22; 8 <= H <= "
                  "4096, a multiple of 8; x_dtype TMI_F32 or TMI_BF16; x_st >= H, m_st >= H, item strides >= T_max * the frame "
                  "stride, all <= 2^30; 1 <= n_src <= 2^30, and >= N without a row_index; layers and its K entries non-NULL, every "
                  "layer and mixed 16-byte aligned; frame_lens, a non-NULL; pointers 4-byte aligned)");
    return TMI_ERR_INVALID;
  }
  const rows_t g = lm_rows_of(x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max);
  const bool m_vec = m_sn % 4 == 0 && m_st % 4 == 0;
  const int64_t threads = N * T_max * (H / 8);
  const dim3 grid((unsigned)((threads + LM_THREADS - 1) / LM_THREADS));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (x_dtype == TMI_BF16)
    hipLaunchKernelGGL(layer_mix_fwd_kernel<bf16_t>, grid, dim3(LM_THREADS), 0, st, L, (int)K, g, a, w_out, mixed, m_sn, m_st, m_vec,
                       (int)H);
  else
    hipLaunchKernelGGL(layer_mix_fwd_kernel<float>, grid, dim3(LM_THREADS), 0, st, L, (int)K, g, a, w_out, mixed, m_sn, m_st, m_vec,
                       (int)H);
  return tmi_check_launch("tmi_layer_mix_fwd");
}

extern "C" int tmi_layer_mix_fwd(const void* const* layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                 const int32_t* row_index, const int32_t* frame_lens, const float* a, float* w_out, float* mixed,
                                 int64_t m_sn, int64_t m_st, int64_t N, int64_t T_max, int64_t H, void* stream) {
  return tmi_plan_run<tmi_layer_mix_fwd_impl>(lm_layers_of(layers, K), layers != nullptr, K, x_dtype, x_sn, x_st, n_src, row_index,
                                              frame_lens, a, w_out, mixed, m_sn, m_st, N, T_max, H, stream);
}

template <typename T, int KM, typename... A>
static void lm_launch_bwd(bool masked, dim3 grid, hipStream_t st, A... a) {
  if (masked) hipLaunchKernelGGL((layer_mix_bwd_kernel<T, KM, true>), grid, dim3(LM_THREADS), 0, st, a...);
  else hipLaunchKernelGGL((layer_mix_bwd_kernel<T, KM, false>), grid, dim3(LM_THREADS), 0, st, a...);
}
template <typename T, typename... A>
static void lm_launch_bwd_k(int64_t K, bool masked, dim3 grid, hipStream_t st, A... a) {
  if (K <= 8) lm_launch_bwd<T, 8>(masked, grid, st, a...);
  else if (K <= 16) lm_launch_bwd<T, 16>(masked, grid, st, a...);
  else if (K <= 32) lm_launch_bwd<T, 32>(masked, grid, st, a...);
  else lm_launch_bwd<T, 64>(masked, grid, st, a...);
}

static int tmi_layer_mix_bwd_impl(layers_t L, bool have_layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st,
                                  int64_t n_src, const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens,
                                  const float* grad, int64_t gr_sn, int64_t gr_st, const int32_t* infeasible, float p, uint64_t seed,
                                  int32_t reduction, const float* W, const float* a, float* g_a, float* d, void* workspace,
                                  int64_t workspace_bytes, int64_t N, int64_t T_max, int64_t L_max, int64_t H, int64_t V,
                                  const uint32_t* time_bits, int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* stream) {
  const bool ok = have_layers && lm_sizes_ok(N, T_max, H, K) && lm_v_ok(V) && lm_p_ok(p) &&
                  lm_rows_ok(L, K, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max, H) && f4(label_lens) && f4(grad) &&
                  lm_stride_ok(gr_sn, gr_st, T_max, V) && f4(infeasible) && (reduction == 0 || reduction == 1) && W != nullptr &&
                  tmi_aligned(W, 16) && f4(a) && f4(g_a) && f4n(d) && L_max >= 1 && L_max <= LM_MAXL && workspace != nullptr &&
                  tmi_aligned(workspace, 16) && workspace_bytes >= lm_tiles(N * T_max) * K * 4;
  if (!ok) {
    tmi_set_error("tmi_layer_mix_bwd: bad argument (1 <= K <= 64; the sizes, dtype and strides of tmi_layer_mix_fwd; 2 <= V <= 64; "
                  "0 <= p < 1; gr_st >= V, gr_sn >= T_max * gr_st, both <= 2^30; 1 <= L_max <= 511; reduction 0 (sum) or 1 (mean); "
                  "every pointer but row_index and d non-NULL and 4-byte aligned, the layers and W 16; workspace 16-byte aligned, "
                  "of tmi_layer_mix_workspace_bytes(N, T_max, H, V, K) bytes)");
    return TMI_ERR_INVALID;
  }
  const int64_t lim = (int64_t)1 << 30;
  if (!((time_bits == nullptr || (tmi_aligned(time_bits, 4) && ld_t >= (T_max + 31) / 32 && ld_t <= lim)) &&
        (feat_bits == nullptr || (tmi_aligned(feat_bits, 4) && ld_f >= (H + 31) / 32 && ld_f <= lim)))) {
    tmi_set_error("tmi_layer_mix_bwd_m: bad mask (time_bits / feat_bits NULL or 4-byte aligned uint32 [N][ld], ld_t >= ceil(T_max / "
                  "32), ld_f >= ceil(H / 32), both <= 2^30)");
    return TMI_ERR_INVALID;
  }
  const mask_t mk{time_bits, feat_bits, ld_t, ld_f};
  const bool masked = time_bits != nullptr || feat_bits != nullptr;
  const rows_t g = lm_rows_of(x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max);
  drop_t drop;
  drop.on = p > 0.f;
  drop.key = tmi_stream_key(seed, 0);
  drop.thr = tmi_drop_thr(p);
  drop.scale = tmi_keep_scale(drop.thr);
  const int64_t R = N * T_max, tr = lm_tile_rows(R), ntiles = lm_tiles(R);
  float* part = reinterpret_cast<float*>(workspace);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)ntiles);
  if (x_dtype == TMI_BF16)
    lm_launch_bwd_k<bf16_t>(K, masked, grid, st, L, (int)K, g, label_lens, grad, gr_sn, gr_st, infeasible, drop, (int)reduction, W,
                            part, (int)L_max, (int)H, (int)V, (int)tr, mk);
  else
    lm_launch_bwd_k<float>(K, masked, grid, st, L, (int)K, g, label_lens, grad, gr_sn, gr_st, infeasible, drop, (int)reduction, W,
                           part, (int)L_max, (int)H, (int)V, (int)tr, mk);
  const int rc = tmi_check_launch("tmi_layer_mix_bwd");
  if (rc != 0) return rc;
  hipLaunchKernelGGL(layer_mix_fold_kernel, dim3(1), dim3(LM_THREADS), 0, st, part, (int)ntiles, (int)K, a, g_a, d);
  return tmi_check_launch("tmi_layer_mix_bwd");
}

extern "C" int tmi_layer_mix_bwd(const void* const* layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                 const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens, const float* grad,
                                 int64_t gr_sn, int64_t gr_st, const int32_t* infeasible, float p, uint64_t seed, int32_t reduction,
                                 const float* W, const float* a, float* g_a, float* d, void* workspace, int64_t workspace_bytes,
                                 int64_t N, int64_t T_max, int64_t L_max, int64_t H, int64_t V, void* stream) {
  return tmi_plan_run<tmi_layer_mix_bwd_impl>(lm_layers_of(layers, K), layers != nullptr, K, x_dtype, x_sn, x_st, n_src, row_index,
                                              frame_lens, label_lens, grad, gr_sn, gr_st, infeasible, p, tmi_plan_seed{seed},
                                              reduction, W, a, g_a, d, workspace, workspace_bytes, N, T_max, L_max, H, V,
                                              (const uint32_t*)nullptr, (int64_t)0, (const uint32_t*)nullptr, (int64_t)0, stream);
}

extern "C" int tmi_layer_mix_bwd_m(const void* const* layers, int64_t K, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                   const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens, const float* grad,
                                   int64_t gr_sn, int64_t gr_st, const int32_t* infeasible, float p, uint64_t seed, int32_t reduction,
                                   const float* W, const float* a, float* g_a, float* d, void* workspace, int64_t workspace_bytes,
                                   int64_t N, int64_t T_max, int64_t L_max, int64_t H, int64_t V, const uint32_t* time_bits,
                                   int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* stream) {
  return tmi_plan_run<tmi_layer_mix_bwd_impl>(lm_layers_of(layers, K), layers != nullptr, K, x_dtype, x_sn, x_st, n_src, row_index,
                                              frame_lens, label_lens, grad, gr_sn, gr_st, infeasible, p, tmi_plan_seed{seed},
                                              reduction, W, a, g_a, d, workspace, workspace_bytes, N, T_max, L_max, H, V, time_bits,
                                              ld_t, feat_bits, ld_f, stream);
}
