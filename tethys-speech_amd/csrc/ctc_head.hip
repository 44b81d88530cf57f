// The CTC head on cached encoder features (Wav2Vec2ForCTC, V:972-975, trained with the encoder frozen): tmi_ctc_head_fwd,
// tmi_ctc_head_bwd, tmi_ctc_head_workspace_bytes.  include/tethys_mi.h states the contract; this is how it is carried out.
// All arithmetic is fp32, there is no atomic, and every floating-point sum runs in an order fixed by (N, T_max, H, V) and
// the row's position alone, so the same call gives the same bits.  Row r = n * T_max + t is frame t of item n; it is live
// when t < min(frame_lens[n], T_max).  A dead row is never read and never written: it enters a sum as zeros.
//
// ctc_head_fwd_kernel - one workgroup of 256 threads per tile of CT_FR = 16 rows, wave w the rows 4 w .. 4 w + 3, lane l the
//   column l (V <= 64; a lane past V holds no column).  The tile's Dropout(hidden) rows are staged in LDS as fp32, CT_HC =
//   128 columns at a time: a thread loads 8 consecutive elements (one 16-byte load of bf16 when the strides allow it) and
//   draws their 8 keep bits from 4 pair hashes (tmi_drop8).  The same 128 rows of W go to LDS beside them (contiguous in
//   memory, 16-byte loads spread over the workgroup: a thread that walked W row by row from L2 would wait out one load
//   latency per row, which is what bounds tmi_cls_head_fwd).  acc = fmaf(xd[r][h], W[h][l], acc) for h ascending from 0: the
//   xd reads are wave-wide broadcasts, the W reads one bank per lane.  Then logit = acc + b[l] and the row statistics of
//   tmi_ctc_logsoftmax, on the wave: m = the wave maximum, the sum of expf(logit - m) by the xor butterfly 32, 16, .., 1,
//   lse = m + logf(sum), argmax = the lowest lane whose logit equals m (a ballot).
//
// ctc_head_outer_kernel - part[chunk][h][v] = sum over the chunk's rows r ascending of xd[r][h] * gs[r][v] (fmaf from 0) and
//   part[chunk][H][v] = the same sum of gs[r][v] (adds from 0).  A workgroup owns 64 columns of H (all of V: one 64 x 64
//   tile, a thread 4 x 4 of it) for one chunk of `rc` rows and walks them in slices of 32 staged in LDS: xd as the forward
//   forms it, gs = grad * w_n with w_n formed per row from infeasible[n], label_lens[n], N and the reduction.
// ctc_head_fold_kernel - one thread per element of gW and gb adds the chunks' partial sums in ascending chunk order from
//   part[0]; one more workgroup adds the loss (thread t of 256 its items t, t + 256, .. ascending, then block_sum_256) and
//   counts the infeasible items (integers).
//   rc = 256 * ceil(N * T_max / 16384): at most 64 chunks, so the workspace stays at 64 (H V + V) floats however long the
//   batch is; up to 16384 rows a chunk is 256 rows.
//
// SpecAugment (tmi_ctc_head_fwd_m / _bwd_m; the bits of tmi_spec_masks): the forward and the outer kernel are templates on
//   MASKED, and the existing entry points launch the instantiation without it.  With it, a thread that stages a piece reads
//   the time bit of its row (a masked row is not loaded: its xd is zeros) and the byte of the feature word that covers its
//   8 columns, and zeroes xd under it.  Nothing else differs: the sums and their orders are the same.
#include "tmi_common.h"
#include <math.h>
#include <string>

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_FR = 16;        // forward: rows per workgroup (4 per wave)
constexpr int CT_HC = 128;       // forward: columns of hidden (rows of W) staged at a time
constexpr int CT_T = 64;         // backward: tile edge
constexpr int CT_RS = 32;        // backward: rows per slice
constexpr int CT_CR = 256;       // backward: the row chunk is a multiple of this
constexpr int CT_MAXCHUNK = 64;  // backward: chunks at most
constexpr int64_t CT_MAXN = 65535, CT_MAXT = 4096, CT_MAXROWS = (int64_t)1 << 22, CT_MAXH = 4096, CT_MAXV = 64,
                  CT_MAXL = 511;

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
__device__ __forceinline__ bool ct_time_masked(const mask_t& mk, int n, int t) {
  return mk.time_bits != nullptr && ((mk.time_bits[(int64_t)n * mk.ld_t + (t >> 5)] >> (t & 31)) & 1u) != 0;
}
// v[0..8) of item n, columns c .. c + 7 (c a multiple of 8: one byte of a word), zeroed under the feature mask
__device__ __forceinline__ void ct_feat_mask8(const mask_t& mk, int n, int c, float (&v)[8]) {
  if (mk.feat_bits == nullptr) return;
  const uint32_t m = (mk.feat_bits[(int64_t)n * mk.ld_f + (c >> 5)] >> (c & 31)) & 0xffu;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((m >> k) & 1u) v[k] = 0.f;
}

struct rows_t {  // what locates a row: the same in every kernel
  int64_t x_sn, x_st, n_src;
  const int32_t* row_index;
  const int32_t* frame_lens;
  int N, T_max;
  bool vec;  // 16-byte loads of 8 elements are aligned
};

// frames of item n (device values are not trusted: clamped to [0, T_max])
__device__ __forceinline__ int ct_frames(const rows_t& g, int n) {
  const int f = g.frame_lens[n];
  return f < 0 ? 0 : (f > g.T_max ? g.T_max : f);
}
// the source item of position n (-1: a row_index entry outside [0, n_src) reads as zeros)
__device__ __forceinline__ int64_t ct_src(const rows_t& g, int n) {
  const int64_t s = g.row_index ? (int64_t)g.row_index[n] : (int64_t)n;
  return (s >= 0 && s < g.n_src) ? s : -1;
}

// xd[0..8) of row r (frame t of source item s >= 0), columns c .. c + 7 (c a multiple of 8)
template <typename T>
__device__ __forceinline__ void ct_load8(const T* __restrict__ hidden, const rows_t& g, const drop_t& d, int64_t s, int t, int r,
                                         int c, float (&v)[8]) {
  const T* __restrict__ p = hidden + s * g.x_sn + (int64_t)t * g.x_st + c;
  if constexpr (sizeof(T) == 2) {
    if (g.vec) {
      const bf16x8 q = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (float)q[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = to_f32(p[k]);
    }
  } else {
    if (g.vec) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = a[k], v[4 + k] = b[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = to_f32(p[k]);
    }
  }
  if (d.on) tmi_drop8(v, r, c, d.key, d.thr, d.scale);
}

template <typename T, bool MASKED>
__global__ __launch_bounds__(CT_THREADS) void ctc_head_fwd_kernel(const T* __restrict__ hidden, rows_t g,
                                                                 const float* __restrict__ W, const float* __restrict__ b,
                                                                 drop_t drop, float* __restrict__ logits, int64_t lg_sn,
                                                                 int64_t lg_st, float* __restrict__ logp, int64_t lp_sn,
                                                                 int64_t lp_st, int32_t* __restrict__ amax, int H, int V, mask_t mk) {
  __shared__ __attribute__((aligned(16))) float xs[CT_FR][CT_HC];
  __shared__ __attribute__((aligned(16))) float Ws[CT_HC * 64];  // the slice's rows of W, [hl][V] as in memory
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int R = g.N * g.T_max, r0 = blockIdx.x * CT_FR;
  // the 8-element piece this thread stages per slice: row tid / 16, columns (tid % 16) * 8
  const int sr = tid >> 4, sc = (tid & 15) * 8;
  int st_t = 0, st_n = 0;
  int64_t st_s = -1;
  if (r0 + sr < R) {
    const int r = r0 + sr, n = r / g.T_max, t = r - n * g.T_max;
    if (t < ct_frames(g, n)) st_s = ct_src(g, n), st_t = t;
    if constexpr (MASKED) {
      st_n = n;
      if (st_s >= 0 && ct_time_masked(mk, n, t)) st_s = -1;  // a time-masked row is not loaded
    }
  }
  // the four rows of this wave (uniform over it)
  bool live[4], any = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = r0 + wv * 4 + j;
    live[j] = false;
    if (r < R) {
      const int n = r / g.T_max;
      live[j] = r - n * g.T_max < ct_frames(g, n);
    }
    any = any || live[j];
  }
  const bool in = lane < V;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int h0 = 0; h0 < H; h0 += CT_HC) {
    const int hl = H - h0 < CT_HC ? H - h0 : CT_HC;  // (a multiple of 8)
    __syncthreads();
    if (sc < hl) {
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (st_s >= 0) {
        ct_load8(hidden, g, drop, st_s, st_t, r0 + sr, h0 + sc, v);
        if constexpr (MASKED) ct_feat_mask8(mk, st_n, h0 + sc, v);
      }
      *reinterpret_cast<f32x4*>(&xs[sr][sc]) = f32x4{v[0], v[1], v[2], v[3]};
      *reinterpret_cast<f32x4*>(&xs[sr][sc + 4]) = f32x4{v[4], v[5], v[6], v[7]};
    }
    {  // hl * V floats of W, contiguous from row h0 (16-byte aligned: W is, h0 is a multiple of 128, hl * V of 8)
      const f32x4* __restrict__ src = reinterpret_cast<const f32x4*>(W + (int64_t)h0 * V);
      for (int e = tid; e < hl * V / 4; e += CT_THREADS) reinterpret_cast<f32x4*>(Ws)[e] = src[e];
    }
    __syncthreads();
    if (!any) continue;  // (uniform over the wave; the barriers above are reached by every thread)
    for (int hh = 0; hh < hl; hh += 4) {
      f32x4 xv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[j] = *reinterpret_cast<const f32x4*>(&xs[wv * 4 + j][hh]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float w = in ? Ws[(hh + k) * V + lane] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(xv[j][k], w, acc[j]);
      }
    }
  }
  const float bias = in ? b[lane] : 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!live[j]) continue;  // (uniform over the wave)
    const int r = r0 + wv * 4 + j, n = r / g.T_max, t = r - n * g.T_max;
    const float v = in ? acc[j] + bias : -INFINITY;
    const float m = wave_max(v);
    const float e = in ? expf(v - m) : 0.f;
    const float lse = m + logf(wave_sum(e));
    if (in) {
      logp[(int64_t)n * lp_sn + (int64_t)t * lp_st + lane] = v - lse;
      if (logits != nullptr) logits[(int64_t)n * lg_sn + (int64_t)t * lg_st + lane] = v;
    }
    const unsigned long long eq = __ballot(in && v == m);
    if (lane == 0 && amax != nullptr) amax[r] = eq ? (int32_t)__builtin_ctzll(eq) : 0;
  }
}

// w_n of a feasible item: 1 ("sum") or 1 / (max(L, 1) * N) ("mean"), L clamped to [0, L_max]
__device__ __forceinline__ float ct_weight(const int32_t* __restrict__ label_lens, int n, int N, int L_max, int reduction) {
  if (reduction == 0) return 1.0f;
  int L = label_lens[n];
  L = L < 1 ? 1 : (L > L_max ? L_max : L);
  return 1.0f / ((float)L * (float)N);
}

template <typename T, bool MASKED>
__global__ __launch_bounds__(CT_THREADS) void ctc_head_outer_kernel(const T* __restrict__ hidden, rows_t g,
                                                                   const int32_t* __restrict__ label_lens,
                                                                   const float* __restrict__ grad, int64_t gr_sn, int64_t gr_st,
                                                                   const int32_t* __restrict__ infeasible, drop_t drop,
                                                                   int reduction, float* __restrict__ part, int L_max, int H,
                                                                   int V, int rc, mask_t mk) {
  __shared__ __attribute__((aligned(16))) float As[CT_RS][CT_T];
  __shared__ __attribute__((aligned(16))) float Bs[CT_RS][CT_T];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int i0 = blockIdx.x * CT_T;
  const int R = g.N * g.T_max;
  const int row_lo = blockIdx.y * rc, row_hi = row_lo + rc < R ? row_lo + rc : R;
  float* __restrict__ out = part + (int64_t)blockIdx.y * ((int64_t)H * V + V);
  float acc[4][4], cs[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    cs[a] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = 0.f;
  }
  const int rr = tid >> 3, c8 = (tid & 7) * 8;  // the piece of a slice this thread stages: row rr, columns c8 .. c8 + 7
  for (int rb = row_lo; rb < row_hi; rb += CT_RS) {
    __syncthreads();
    {
      float av[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const int r = rb + rr;
      if (r < row_hi) {
        const int n = r / g.T_max, t = r - n * g.T_max;
        if (t < ct_frames(g, n)) {
          const int64_t s = ct_src(g, n);
          if constexpr (MASKED) {
            if (s >= 0 && i0 + c8 < H && !ct_time_masked(mk, n, t)) {
              ct_load8(hidden, g, drop, s, t, r, i0 + c8, av);
              ct_feat_mask8(mk, n, i0 + c8, av);
            }
          } else {
            if (s >= 0 && i0 + c8 < H) ct_load8(hidden, g, drop, s, t, r, i0 + c8, av);
          }
          const float w = infeasible[n] != 0 ? 0.f : ct_weight(label_lens, n, g.N, L_max, reduction);
          const float* __restrict__ gp = grad + (int64_t)n * gr_sn + (int64_t)t * gr_st;
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (c8 + q < V) bv[q] = gp[c8 + q] * w;
        }
      }
      *reinterpret_cast<f32x4*>(&As[rr][c8]) = f32x4{av[0], av[1], av[2], av[3]};
      *reinterpret_cast<f32x4*>(&As[rr][c8 + 4]) = f32x4{av[4], av[5], av[6], av[7]};
      *reinterpret_cast<f32x4*>(&Bs[rr][c8]) = f32x4{bv[0], bv[1], bv[2], bv[3]};
      *reinterpret_cast<f32x4*>(&Bs[rr][c8 + 4]) = f32x4{bv[4], bv[5], bv[6], bv[7]};
    }
    __syncthreads();
    const int nr = row_hi - rb < CT_RS ? row_hi - rb : CT_RS;
    for (int q = 0; q < nr; ++q) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&As[q][ti * 4]);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[q][tj * 4]);
#pragma unroll
      for (int c = 0; c < 4; ++c) cs[c] += bv[c];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][c] = fmaf(av[a], bv[c], acc[a][c]);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ti * 4 + a;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = tj * 4 + c;
      if (i < H && j < V) out[(int64_t)i * V + j] = acc[a][c];
    }
  }
  if (blockIdx.x == 0 && ti == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = tj * 4 + c;
      if (j < V) out[(int64_t)H * V + j] = cs[c];
    }
  }
}

// gW | gb [e] = part[0][e] + part[1][e] + .. in that order, e < n_out; the last workgroup: the loss and the count
__global__ __launch_bounds__(CT_THREADS) void ctc_head_fold_kernel(const float* __restrict__ part, int nchunk, int64_t n_w,
                                                                  int64_t n_out, float* __restrict__ gW, float* __restrict__ gb,
                                                                  const float* __restrict__ nll,
                                                                  const int32_t* __restrict__ infeasible,
                                                                  const int32_t* __restrict__ label_lens, int N, int L_max,
                                                                  int reduction, float* __restrict__ loss,
                                                                  int32_t* __restrict__ n_infeasible) {
  __shared__ float red[4];
  __shared__ int redi[4];
  if (blockIdx.x + 1 == gridDim.x) {
    float s = 0.f;
    int cnt = 0;
    for (int n = threadIdx.x; n < N; n += CT_THREADS) {
      if (infeasible[n] != 0) cnt += 1;
      else s += ct_weight(label_lens, n, N, L_max, reduction) * nll[n];
    }
    s = block_sum_256(s, red);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      loss[0] = s;
      n_infeasible[0] = redi[0] + redi[1] + redi[2] + redi[3];
    }
    return;
  }
  const int64_t e = (int64_t)blockIdx.x * CT_THREADS + threadIdx.x;
  if (e >= n_out) return;
  float s = part[e];
  for (int k = 1; k < nchunk; ++k) s += part[(int64_t)k * n_out + e];
  if (e < n_w) gW[e] = s;
  else gb[e - n_w] = s;
}

bool ct_sizes_ok(int64_t N, int64_t T_max, int64_t H, int64_t V) {
  return N >= 1 && N <= CT_MAXN && T_max >= 1 && T_max <= CT_MAXT && N * T_max <= CT_MAXROWS && H >= 8 && H <= CT_MAXH &&
         H % 8 == 0 && V >= 2 && V <= CT_MAXV;
}
int64_t ct_chunk_rows(int64_t R) { return CT_CR * ((R + (int64_t)CT_CR * CT_MAXCHUNK - 1) / ((int64_t)CT_CR * CT_MAXCHUNK)); }
int64_t ct_chunks(int64_t R) { return (R + ct_chunk_rows(R) - 1) / ct_chunk_rows(R); }
bool ct_p_ok(float p) { return p >= 0.f && p < 1.f && tmi_drop_ok(p); }
bool ct_stride_ok(int64_t sn, int64_t st, int64_t T_max, int64_t cols) {
  const int64_t lim = (int64_t)1 << 30;
  return st >= cols && st <= lim && sn >= T_max * st && sn <= lim;
}
bool ct_rows_ok(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index,
                const int32_t* frame_lens, int64_t N, int64_t T_max, int64_t H) {
  return hidden != nullptr && tmi_aligned(hidden, 16) && (x_dtype == TMI_F32 || x_dtype == TMI_BF16) &&
         ct_stride_ok(x_sn, x_st, T_max, H) && n_src >= 1 && n_src <= ((int64_t)1 << 30) && (row_index != nullptr || n_src >= N) &&
         tmi_aligned(row_index, 4) && frame_lens != nullptr && tmi_aligned(frame_lens, 4);
}
rows_t ct_rows_of(int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src, const int32_t* row_index, const int32_t* frame_lens,
                  int64_t N, int64_t T_max) {
  rows_t g;
  g.x_sn = x_sn, g.x_st = x_st, g.n_src = n_src, g.row_index = row_index, g.frame_lens = frame_lens;
  g.N = (int)N, g.T_max = (int)T_max;
  const int64_t q = x_dtype == TMI_BF16 ? 8 : 4;  // elements per 16 bytes
  g.vec = x_sn % q == 0 && x_st % q == 0;
  return g;
}
drop_t ct_drop_of(float p, uint64_t seed) {
  drop_t d;
  d.on = p > 0.f;
  d.key = tmi_stream_key(seed, 0);
  d.thr = tmi_drop_thr(p);
  d.scale = tmi_keep_scale(d.thr);
  return d;
}
// (NULL: that mask is off and its ld is not looked at)
bool ct_mask_ok(const uint32_t* time_bits, int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, int64_t T_max, int64_t H) {
  const int64_t lim = (int64_t)1 << 30;
  return (time_bits == nullptr || (tmi_aligned(time_bits, 4) && ld_t >= (T_max + 31) / 32 && ld_t <= lim)) &&
         (feat_bits == nullptr || (tmi_aligned(feat_bits, 4) && ld_f >= (H + 31) / 32 && ld_f <= lim));
}
const char* const ct_mask_msg = ": bad mask (time_bits / feat_bits NULL or 4-byte aligned uint32 [N][ld], ld_t >= ceil(T_max / 32), "
                                "ld_f >= ceil(H / 32), both <= 2^30)";
inline bool f4(const void* p) { return p != nullptr && tmi_aligned(p, 4); }
inline bool f4n(const void* p) { return tmi_aligned(p, 4); }  // (may be NULL)

}  // namespace

extern "C" int64_t tmi_ctc_head_workspace_bytes(int64_t N, int64_t T_max, int64_t H, int64_t V) {
  if (!ct_sizes_ok(N, T_max, H, V)) return -1;
  return ct_chunks(N * T_max) * (H * V + V) * 4;
}

static int tmi_ctc_head_fwd_impl(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                 const int32_t* row_index, const int32_t* frame_lens, const float* W, const float* b, float p,
                                 uint64_t seed, float* logits, int64_t lg_sn, int64_t lg_st, float* logp, int64_t lp_sn,
                                 int64_t lp_st, int32_t* argmax, int64_t N, int64_t T_max, int64_t H, int64_t V,
                                 const uint32_t* time_bits, int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* stream) {
  const bool ok = ct_sizes_ok(N, T_max, H, V) && ct_p_ok(p) &&
                  ct_rows_ok(hidden, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max, H) && W != nullptr &&
                  tmi_aligned(W, 16) && f4(b) && f4(logp) && ct_stride_ok(lp_sn, lp_st, T_max, V) && f4n(logits) &&
                  (logits == nullptr || ct_stride_ok(lg_sn, lg_st, T_max, V)) && f4n(argmax);
  if (!ok) {
    tmi_set_error("tmi_ctc_head_fwd: bad argument (1 <= N <= 65535; 1 <= T_max <= 4096; N*T_max <= 2^22; 8 <= H <= 4096, a "
                  "multiple of 8; 2 <= V <= 64; 0 <= p < 1; x_dtype TMI_F32 or TMI_BF16; x_st >= H, lg_st >= V, lp_st >= V, item "
                  "strides >= T_max * the frame stride, all <= 2^30; 1 <= n_src <= 2^30, and >= N without a row_index; hidden and "
                  "W non-NULL and 16-byte aligned; frame_lens, b, logp non-NULL; pointers 4-byte aligned)");
    return TMI_ERR_INVALID;
  }
  if (!ct_mask_ok(time_bits, ld_t, feat_bits, ld_f, T_max, H)) {
    tmi_set_error((std::string("tmi_ctc_head_fwd_m") + ct_mask_msg).c_str());
    return TMI_ERR_INVALID;
  }
  const rows_t g = ct_rows_of(x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max);
  const mask_t mk{time_bits, feat_bits, ld_t, ld_f};
  const bool masked = time_bits != nullptr || feat_bits != nullptr;
  const dim3 grid((unsigned)((N * T_max + CT_FR - 1) / CT_FR));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const auto launch = [&](auto kernel, auto* x) {
    hipLaunchKernelGGL(kernel, grid, dim3(CT_THREADS), 0, st, x, g, W, b, ct_drop_of(p, seed), logits, lg_sn, lg_st, logp, lp_sn,
                       lp_st, argmax, (int)H, (int)V, mk);
  };
  if (x_dtype == TMI_BF16) {
    const bf16_t* x = reinterpret_cast<const bf16_t*>(hidden);
    if (masked) launch(ctc_head_fwd_kernel<bf16_t, true>, x);
    else launch(ctc_head_fwd_kernel<bf16_t, false>, x);
  } else {
    const float* x = reinterpret_cast<const float*>(hidden);
    if (masked) launch(ctc_head_fwd_kernel<float, true>, x);
    else launch(ctc_head_fwd_kernel<float, false>, x);
  }
  return tmi_check_launch("tmi_ctc_head_fwd");
}

extern "C" int tmi_ctc_head_fwd(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                const int32_t* row_index, const int32_t* frame_lens, const float* W, const float* b, float p,
                                uint64_t seed, float* logits, int64_t lg_sn, int64_t lg_st, float* logp, int64_t lp_sn,
                                int64_t lp_st, int32_t* argmax, int64_t N, int64_t T_max, int64_t H, int64_t V, void* stream) {
  return tmi_plan_run<tmi_ctc_head_fwd_impl>(hidden, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, W, b, p, tmi_plan_seed{seed},
                                             logits, lg_sn, lg_st, logp, lp_sn, lp_st, argmax, N, T_max, H, V,
                                             (const uint32_t*)nullptr, (int64_t)0, (const uint32_t*)nullptr, (int64_t)0, stream);
}

extern "C" int tmi_ctc_head_fwd_m(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                  const int32_t* row_index, const int32_t* frame_lens, const float* W, const float* b, float p,
                                  uint64_t seed, float* logits, int64_t lg_sn, int64_t lg_st, float* logp, int64_t lp_sn,
                                  int64_t lp_st, int32_t* argmax, int64_t N, int64_t T_max, int64_t H, int64_t V,
                                  const uint32_t* time_bits, int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* stream) {
  return tmi_plan_run<tmi_ctc_head_fwd_impl>(hidden, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, W, b, p, tmi_plan_seed{seed},
                                             logits, lg_sn, lg_st, logp, lp_sn, lp_st, argmax, N, T_max, H, V, time_bits, ld_t,
                                             feat_bits, ld_f, stream);
}

static int tmi_ctc_head_bwd_impl(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                 const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens, const float* grad,
                                 int64_t gr_sn, int64_t gr_st, const float* nll, const int32_t* infeasible, float p, uint64_t seed,
                                 int32_t reduction, float* gW, float* gb, float* loss, int32_t* n_infeasible, void* workspace,
                                 int64_t workspace_bytes, int64_t N, int64_t T_max, int64_t L_max, int64_t H, int64_t V,
                                 const uint32_t* time_bits, int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* stream) {
  const bool ok = ct_sizes_ok(N, T_max, H, V) && ct_p_ok(p) &&
                  ct_rows_ok(hidden, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max, H) && f4(label_lens) && f4(grad) &&
                  ct_stride_ok(gr_sn, gr_st, T_max, V) && f4(nll) && f4(infeasible) && (reduction == 0 || reduction == 1) &&
                  f4(gW) && f4(gb) && f4(loss) && f4(n_infeasible) && L_max >= 1 && L_max <= CT_MAXL && workspace != nullptr &&
                  tmi_aligned(workspace, 16) && workspace_bytes >= ct_chunks(N * T_max) * (H * V + V) * 4;
  if (!ok) {
    tmi_set_error("tmi_ctc_head_bwd: bad argument (the sizes, p, dtype and strides of tmi_ctc_head_fwd; gr_st >= V, gr_sn >= "
                  "T_max * gr_st, both <= 2^30; 1 <= L_max <= 511; reduction 0 (sum) or 1 (mean); every pointer but row_index "
                  "non-NULL and 4-byte aligned, hidden 16; workspace 16-byte aligned, of tmi_ctc_head_workspace_bytes(N, T_max, H, "
                  "V) bytes)");
    return TMI_ERR_INVALID;
  }
  if (!ct_mask_ok(time_bits, ld_t, feat_bits, ld_f, T_max, H)) {
    tmi_set_error((std::string("tmi_ctc_head_bwd_m") + ct_mask_msg).c_str());
    return TMI_ERR_INVALID;
  }
  const rows_t g = ct_rows_of(x_dtype, x_sn, x_st, n_src, row_index, frame_lens, N, T_max);
  const drop_t drop = ct_drop_of(p, seed);
  const mask_t mk{time_bits, feat_bits, ld_t, ld_f};
  const bool masked = time_bits != nullptr || feat_bits != nullptr;
  const int64_t R = N * T_max, rc = ct_chunk_rows(R), nchunk = ct_chunks(R);
  float* part = reinterpret_cast<float*>(workspace);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)((H + CT_T - 1) / CT_T), (unsigned)nchunk);
  const auto launch = [&](auto kernel, auto* x) {
    hipLaunchKernelGGL(kernel, grid, dim3(CT_THREADS), 0, st, x, g, label_lens, grad, gr_sn, gr_st, infeasible, drop, (int)reduction,
                       part, (int)L_max, (int)H, (int)V, (int)rc, mk);
  };
  if (x_dtype == TMI_BF16) {
    const bf16_t* x = reinterpret_cast<const bf16_t*>(hidden);
    if (masked) launch(ctc_head_outer_kernel<bf16_t, true>, x);
    else launch(ctc_head_outer_kernel<bf16_t, false>, x);
  } else {
    const float* x = reinterpret_cast<const float*>(hidden);
    if (masked) launch(ctc_head_outer_kernel<float, true>, x);
    else launch(ctc_head_outer_kernel<float, false>, x);
  }
  int rc_launch = tmi_check_launch("tmi_ctc_head_bwd");
  if (rc_launch != 0) return rc_launch;
  const int64_t n_out = H * V + V;
  hipLaunchKernelGGL(ctc_head_fold_kernel, dim3((unsigned)((n_out + CT_THREADS - 1) / CT_THREADS) + 1), dim3(CT_THREADS), 0, st, part,
                     (int)nchunk, H * V, n_out, gW, gb, nll, infeasible, label_lens, (int)N, (int)L_max, (int)reduction, loss,
                     n_infeasible);
  return tmi_check_launch("tmi_ctc_head_bwd");
}

extern "C" int tmi_ctc_head_bwd(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens, const float* grad,
                                int64_t gr_sn, int64_t gr_st, const float* nll, const int32_t* infeasible, float p, uint64_t seed,
                                int32_t reduction, float* gW, float* gb, float* loss, int32_t* n_infeasible, void* workspace,
                                int64_t workspace_bytes, int64_t N, int64_t T_max, int64_t L_max, int64_t H, int64_t V,
                                void* stream) {
  return tmi_plan_run<tmi_ctc_head_bwd_impl>(hidden, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, label_lens, grad, gr_sn,
                                             gr_st, nll, infeasible, p, tmi_plan_seed{seed}, reduction, gW, gb, loss, n_infeasible,
                                             workspace, workspace_bytes, N, T_max, L_max, H, V, (const uint32_t*)nullptr,
                                             (int64_t)0, (const uint32_t*)nullptr, (int64_t)0, stream);
}

extern "C" int tmi_ctc_head_bwd_m(const void* hidden, int32_t x_dtype, int64_t x_sn, int64_t x_st, int64_t n_src,
                                  const int32_t* row_index, const int32_t* frame_lens, const int32_t* label_lens, const float* grad,
                                  int64_t gr_sn, int64_t gr_st, const float* nll, const int32_t* infeasible, float p, uint64_t seed,
                                  int32_t reduction, float* gW, float* gb, float* loss, int32_t* n_infeasible, void* workspace,
                                  int64_t workspace_bytes, int64_t N, int64_t T_max, int64_t L_max, int64_t H, int64_t V,
                                  const uint32_t* time_bits, int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* stream) {
  return tmi_plan_run<tmi_ctc_head_bwd_impl>(hidden, x_dtype, x_sn, x_st, n_src, row_index, frame_lens, label_lens, grad, gr_sn,
                                             gr_st, nll, infeasible, p, tmi_plan_seed{seed}, reduction, gW, gb, loss, n_infeasible,
                                             workspace, workspace_bytes, N, T_max, L_max, H, V, time_bits, ld_t, feat_bits, ld_f,
                                             stream);
}
