// The sequence-classification head (Wav2Vec2ForSequenceClassification, V:1045-1056): tmi_cls_head_fwd, tmi_cls_head_bwd,
// tmi_cls_head_workspace_bytes.  include/tethys_mi.h states the contract; this is how it is carried out.  All arithmetic is
// fp32; the only atomics are the integer adds of the confusion table; every floating-point sum runs in an order fixed by
// (H, P, C) and the row's position alone, so the same call gives the same bits.
//
// cls_fwd_kernel - one workgroup of 256 threads per tile of CH_TR = 8 rows, so Wp is read once per 8 rows.  LDS (dynamic):
//   ys[8][P], the tile's Dropout(tanh(.)) between the two products, and a second region that holds first the tile's slice
//   x[8][256] of the (gathered) pooled rows, then the tile's logits[8][C].
//   product 1: thread t owns columns t, t + 256, .. of P; for h ascending in slices of 256, acc = fmaf(x[r][h], Wp[h][c], acc)
//     from 0; pre = acc + bp[c]; z = tanhf(pre); y = keep(seed, r, c) ? z * scale : 0 (p == 0: y = z, nothing is hashed).
//   product 2: thread t owns classes t, t + 256, ..; acc = fmaf(y[r][q], Wc[q][c], acc) for q ascending from 0; + bc[c].
//   row statistics: wave w serves rows w and w + 4, lane l the classes l, l + 64, .. in ascending order, then a butterfly:
//     m = max; s = sum of expf(logit - m) (lane partial sums ascending, then the xor butterfly 32, 16, .., 1);
//     lse = m + logf(s); log_probs[c] = logit[c] - lse; nll = -(logit[label] - lse); pred and label_rank are integer
//     reductions (exact).
//
// cls_count_kernel - one workgroup: n_valid and the mean loss.  Thread t adds the rows t, t + 256, .. in ascending order,
//   then block_sum_256.  It leaves n_valid and 1 / n_valid (0 when nothing is labelled) in the workspace header.
// cls_dpre_kernel - one workgroup per 8 rows: dlogits of the tile in LDS, thread t owns columns t, t + 256, .. of P:
//   acc = fmaf(dlogits[r][c], Wc[q][c], acc) for c ascending; dpre = (keep ? acc * scale : 0) * fmaf(-z, z, 1).
// cls_outer_kernel - out[i][j] = sum over rows r ascending of A[r][i] * B[r][j] (fmaf from 0), colsum[j] = sum_r B[r][j]:
//   MODE 0: A = y (z and the mask again), B = dlogits (log_probs and labels again) -> gWc, gbc
//   MODE 1: A = the gathered pooled rows, B = dpre                                 -> gWp, gbp
//   A workgroup owns a 64 x 64 tile of `out` for one CHUNK of CO_CR = 256 rows (blockIdx.z), a thread 4 x 4 of it, and walks
//   the chunk's rows in ascending order in slices of 32 staged in LDS.  N <= 256: the one chunk writes `out` itself.
//   N > 256: every chunk writes its partial sums to the workspace and cls_fold_kernel adds the chunks in ascending order,
//   one thread per element: the order is fixed by N alone, there is no atomic.
//
// gWp is computed in this file, not as a tmi_gemm with transposed strides: tmi_gemm has no gather, so with a row_index it
// would need a gathered copy of the rows first, and its split-K order is its tile choice's, not the row order stated in the
// header.  Measured both ways on one MI355X (tools/cls_head_bench.py, profiles/r25_cls_head.json "gwp"; H 768, P 256, C 2):
// the whole backward call takes 19.4 us at N 8 and 132.7 us at N 4096, of which this product is 0.4 us and 31.9 us (the
// call at H 768 minus the call at H 4); one exact-fp32 tmi_gemm with transposed strides takes 23.0 us and 297.9 us.
#include "tmi_common.h"
#include <math.h>

namespace {

constexpr int CH_TR = 8;        // rows per workgroup (fwd, dpre)
constexpr int CH_HC = 256;      // columns of pooled staged at a time
constexpr int CH_THREADS = 256;
constexpr int CH_MAXH = 4096, CH_MAXP = 1024, CH_MAXC = 1024;
constexpr int64_t CH_MAXN = 65535;
constexpr int CH_HDR = 256;     // workspace header bytes: [0] n_valid (int32), [1] 1 / n_valid (float)
constexpr int CO_T = 64;        // outer-product tile edge
constexpr int CO_RC = 32;       // rows per slice
constexpr int CO_CR = 256;      // rows per chunk (one workgroup of the outer-product kernel)

struct drop_t {
  uint32_t key, thr;
  float scale;
  bool on;
};
__device__ __forceinline__ float ch_drop(const drop_t& d, float v, uint32_t r, uint32_t c) {
  if (!d.on) return v;
  return tmi_keep(d.key, r, c, d.thr) ? v * d.scale : 0.f;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the source row of position r (-1: a row_index entry outside [0, n_src) reads as a row of zeros)
__device__ __forceinline__ int64_t ch_src(const int32_t* __restrict__ row_index, int64_t r, int64_t n_src) {
  const int64_t s = row_index ? (int64_t)row_index[r] : r;
  return (s >= 0 && s < n_src) ? s : -1;
}

__global__ __launch_bounds__(CH_THREADS) void cls_fwd_kernel(
    const float* __restrict__ pooled, int64_t ld_x, int64_t n_src, const int32_t* __restrict__ row_index,
    const float* __restrict__ Wp, const float* __restrict__ bp, const float* __restrict__ Wc, const float* __restrict__ bc,
    const int32_t* __restrict__ labels, drop_t drop, float* __restrict__ logits, int64_t ld_lg, int32_t* __restrict__ pred,
    float* __restrict__ zout, int64_t ld_z, float* __restrict__ log_probs, int64_t ld_lp, float* __restrict__ nll,
    int32_t* __restrict__ label_rank, unsigned long long* confusion, int64_t ld_cf, int N, int H, int P, int C) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* ys = smem;                      // [CH_TR][P]
  float* xs = smem + CH_TR * P;          // [CH_TR][CH_HC], then the logits [CH_TR][C]
  const int LS = C > CH_HC ? C : CH_HC;  // (row stride of the logits in that region)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int r0 = blockIdx.x * CH_TR;

  // ---- product 1
  float acc[4][CH_TR];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < CH_TR; ++r) acc[j][r] = 0.f;
  for (int h0 = 0; h0 < H; h0 += CH_HC) {
    const int hl = H - h0 < CH_HC ? H - h0 : CH_HC;  // (a multiple of 4)
    __syncthreads();
    for (int e = tid; e < CH_TR * CH_HC; e += CH_THREADS) {
      const int r = e / CH_HC, hh = e % CH_HC;
      float v = 0.f;
      if (r0 + r < N && hh < hl) {
        const int64_t s = ch_src(row_index, r0 + r, n_src);
        if (s >= 0) v = pooled[s * ld_x + h0 + hh];
      }
      xs[e] = v;
    }
    __syncthreads();
    for (int hh = 0; hh < hl; hh += 4) {
      f32x4 xv[CH_TR];
#pragma unroll
      for (int r = 0; r < CH_TR; ++r) xv[r] = *reinterpret_cast<const f32x4*>(xs + r * CH_HC + hh);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float* __restrict__ wrow = Wp + (int64_t)(h0 + hh + k) * P;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = tid + j * CH_THREADS;
          if (c < P) {
            const float w = wrow[c];
#pragma unroll
            for (int r = 0; r < CH_TR; ++r) acc[j][r] = fmaf(xv[r][k], w, acc[j][r]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = tid + j * CH_THREADS;
    if (c < P) {
      const float b = bp[c];
#pragma unroll
      for (int r = 0; r < CH_TR; ++r) {
        const float z = tanhf(acc[j][r] + b);
        const bool live = r0 + r < N;
        if (zout != nullptr && live) zout[(int64_t)(r0 + r) * ld_z + c] = z;
        ys[r * P + c] = live ? ch_drop(drop, z, (uint32_t)(r0 + r), (uint32_t)c) : 0.f;
      }
    }
  }
  __syncthreads();  // (ys complete; every thread has left xs)

  // ---- product 2
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < CH_TR; ++r) acc[j][r] = 0.f;
  for (int q = 0; q < P; ++q) {
    float yv[CH_TR];
#pragma unroll
    for (int r = 0; r < CH_TR; ++r) yv[r] = ys[r * P + q];
    const float* __restrict__ wrow = Wc + (int64_t)q * C;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = tid + j * CH_THREADS;
      if (c < C) {
        const float w = wrow[c];
#pragma unroll
        for (int r = 0; r < CH_TR; ++r) acc[j][r] = fmaf(yv[r], w, acc[j][r]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = tid + j * CH_THREADS;
    if (c < C) {
      const float b = bc[c];
#pragma unroll
      for (int r = 0; r < CH_TR; ++r) {
        const float v = acc[j][r] + b;
        xs[r * LS + c] = v;
        if (r0 + r < N) logits[(int64_t)(r0 + r) * ld_lg + c] = v;
      }
    }
  }
  __syncthreads();

  // ---- row statistics: wave wv serves rows wv and wv + 4
  for (int r = wv; r < CH_TR; r += CH_THREADS / TMI_WAVE) {
    const int row = r0 + r;
    if (row >= N) break;  // (uniform over the wave)
    const float* __restrict__ lg = xs + r * LS;
    float m = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
      const float v = lg[c];
      if (v > m || bi == 0x7fffffff) m = v, bi = c;  // (the lane's first class, then strictly greater: the lowest index)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || om > m || (om == m && oi < bi))) m = om, bi = oi;
    }
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(lg[c] - m);
    s = wave_sum(s);
    const float lse = m + logf(s);
    if (log_probs != nullptr)
      for (int c = lane; c < C; c += 64) log_probs[(int64_t)row * ld_lp + c] = lg[c] - lse;
    const int lab = labels != nullptr ? labels[row] : -1;
    const bool valid = lab >= 0 && lab < C;
    int rank = 0;
    float ll = 0.f;
    if (valid) {
      ll = lg[lab];
      for (int c = lane; c < C; c += 64) {
        const float v = lg[c];
        rank += (v > ll || (v == ll && c < lab)) ? 1 : 0;
      }
      rank = wave_sum_i(rank);
    }
    if (lane == 0) {
      pred[row] = bi;
      if (nll != nullptr) nll[row] = valid ? -(ll - lse) : 0.f;
      if (label_rank != nullptr) label_rank[row] = valid ? rank : -1;
      if (confusion != nullptr && valid) atomicAdd(confusion + (int64_t)lab * ld_cf + bi, 1ull);
    }
  }
}

__global__ __launch_bounds__(CH_THREADS) void cls_count_kernel(const int32_t* __restrict__ labels,
                                                              const float* __restrict__ log_probs, int64_t ld_lp, int N, int C,
                                                              int32_t* __restrict__ hdr, float* __restrict__ loss) {
  __shared__ float red[4];
  __shared__ int redi[4];
  int cnt = 0;
  float s = 0.f;
  for (int r = threadIdx.x; r < N; r += CH_THREADS) {
    const int lab = labels[r];
    if (lab >= 0 && lab < C) {
      cnt += 1;
      s += -log_probs[(int64_t)r * ld_lp + lab];
    }
  }
  s = block_sum_256(s, red);
  cnt = wave_sum_i(cnt);
  if ((threadIdx.x & 63) == 0) redi[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int n = redi[0] + redi[1] + redi[2] + redi[3];
    hdr[0] = n;
    reinterpret_cast<float*>(hdr)[1] = n > 0 ? 1.0f / (float)n : 0.f;
    loss[0] = n > 0 ? s / (float)n : 0.f;
  }
}

// dlogits[r][c] of a labelled row (label `lab` in [0, C)); an unlabelled row has 0 everywhere
__device__ __forceinline__ float ch_dlogit(float lp, int c, int lab, float inv) { return (expf(lp) - (c == lab ? 1.f : 0.f)) * inv; }

__global__ __launch_bounds__(CH_THREADS) void cls_dpre_kernel(const float* __restrict__ Wc, const int32_t* __restrict__ labels,
                                                             drop_t drop, const float* __restrict__ z, int64_t ld_z,
                                                             const float* __restrict__ log_probs, int64_t ld_lp,
                                                             const int32_t* __restrict__ hdr, float* __restrict__ dpre, int N,
                                                             int P, int C) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // dl[CH_TR][C]
  const int tid = threadIdx.x, r0 = blockIdx.x * CH_TR;
  const float inv = reinterpret_cast<const float*>(hdr)[1];
  for (int e = tid; e < CH_TR * C; e += CH_THREADS) {
    const int r = e / C, c = e % C;
    float v = 0.f;
    if (r0 + r < N) {
      const int lab = labels[r0 + r];
      if (lab >= 0 && lab < C) v = ch_dlogit(log_probs[(int64_t)(r0 + r) * ld_lp + c], c, lab, inv);
    }
    smem[e] = v;
  }
  __syncthreads();
  for (int q = tid; q < P; q += CH_THREADS) {
    float acc[CH_TR];
#pragma unroll
    for (int r = 0; r < CH_TR; ++r) acc[r] = 0.f;
    const float* __restrict__ wrow = Wc + (int64_t)q * C;
    for (int c = 0; c < C; ++c) {
      const float w = wrow[c];
#pragma unroll
      for (int r = 0; r < CH_TR; ++r) acc[r] = fmaf(smem[r * C + c], w, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < CH_TR; ++r) {
      if (r0 + r < N) {
        const float zz = z[(int64_t)(r0 + r) * ld_z + q];
        dpre[(int64_t)(r0 + r) * P + q] = ch_drop(drop, acc[r], (uint32_t)(r0 + r), (uint32_t)q) * fmaf(-zz, zz, 1.0f);
      }
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(CH_THREADS) void cls_outer_kernel(
    const float* __restrict__ pooled, int64_t ld_x, int64_t n_src, const int32_t* __restrict__ row_index,
    const int32_t* __restrict__ labels, drop_t drop, const float* __restrict__ z, int64_t ld_z,
    const float* __restrict__ log_probs, int64_t ld_lp, const int32_t* __restrict__ hdr, const float* __restrict__ dpre,
    float* __restrict__ out, float* __restrict__ colsum, float* __restrict__ part, int N, int I, int J, int P) {
  __shared__ __attribute__((aligned(16))) float As[CO_RC][CO_T];
  __shared__ __attribute__((aligned(16))) float Bs[CO_RC][CO_T];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int i0 = blockIdx.x * CO_T, j0 = blockIdx.y * CO_T;
  const float inv = reinterpret_cast<const float*>(hdr)[1];
  float acc[4][4], cs[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    cs[a] = 0.f;
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  }
  const int row_lo = blockIdx.z * CO_CR;
  const int row_hi = row_lo + CO_CR < N ? row_lo + CO_CR : N;
  if (part != nullptr) {  // (more than one chunk: this one's partial sums, [I][J] then [J])
    out = part + (int64_t)blockIdx.z * ((int64_t)I * J + J);
    colsum = out + (int64_t)I * J;
  }
  for (int rb = row_lo; rb < row_hi; rb += CO_RC) {
    __syncthreads();
    for (int e = tid; e < CO_RC * CO_T; e += CH_THREADS) {
      const int rr = e / CO_T, col = e % CO_T, r = rb + rr;
      float av = 0.f, bv = 0.f;
      if (r < row_hi) {
        const int i = i0 + col, j = j0 + col;
        if (MODE == 0) {
          if (i < I) av = ch_drop(drop, z[(int64_t)r * ld_z + i], (uint32_t)r, (uint32_t)i);
          if (j < J) {
            const int lab = labels[r];
            if (lab >= 0 && lab < J) bv = ch_dlogit(log_probs[(int64_t)r * ld_lp + j], j, lab, inv);
          }
        } else {
          if (i < I) {
            const int64_t s = ch_src(row_index, r, n_src);
            if (s >= 0) av = pooled[s * ld_x + i];
          }
          if (j < J) bv = dpre[(int64_t)r * P + j];
        }
      }
      As[rr][col] = av;
      Bs[rr][col] = bv;
    }
    __syncthreads();
    const int nr = row_hi - rb < CO_RC ? row_hi - rb : CO_RC;
    for (int rr = 0; rr < nr; ++rr) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&As[rr][ti * 4]);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(&Bs[rr][tj * 4]);
#pragma unroll
      for (int b = 0; b < 4; ++b) cs[b] += bv[b];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fmaf(av[a], bv[b], acc[a][b]);
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + ti * 4 + a;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tj * 4 + b;
      if (i < I && j < J) out[(int64_t)i * J + j] = acc[a][b];
    }
  }
  if (blockIdx.x == 0 && ti == 0) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int j = j0 + tj * 4 + b;
      if (j < J) colsum[j] = cs[b];
    }
  }
}

// out[e] = part[0][e] + part[1][e] + .. in that order, e < n_out; the same for colsum behind it (chunk stride n_out + n_col)
__global__ __launch_bounds__(CH_THREADS) void cls_fold_kernel(const float* __restrict__ part, int nchunk, int64_t n_out,
                                                             int64_t n_col, float* __restrict__ out, float* __restrict__ colsum) {
  const int64_t e = (int64_t)blockIdx.x * CH_THREADS + threadIdx.x, n = n_out + n_col;
  if (e >= n) return;
  float s = part[e];
  for (int k = 1; k < nchunk; ++k) s += part[(int64_t)k * n + e];
  if (e < n_out) out[e] = s;
  else colsum[e - n_out] = s;
}

// floats of the partial sums behind dpre in the workspace: 0 with one chunk
int64_t ch_part_floats(int64_t N, int64_t H, int64_t P, int64_t C) {
  const int64_t nchunk = (N + CO_CR - 1) / CO_CR;
  if (nchunk <= 1) return 0;
  const int64_t a = H * P + P, b = P * C + C;
  return nchunk * (a > b ? a : b);
}

bool ch_sizes_ok(int64_t N, int64_t H, int64_t P, int64_t C) {
  return N >= 1 && N <= CH_MAXN && H >= 4 && H <= CH_MAXH && H % 4 == 0 && P >= 2 && P <= CH_MAXP && P % 2 == 0 && C >= 1 &&
         C <= CH_MAXC;
}
bool ch_p_ok(float p) { return p >= 0.f && p < 1.f && tmi_drop_ok(p); }
bool ch_rows_ok(int64_t ld_x, int64_t n_src, const int32_t* row_index, int64_t N, int64_t H) {
  const int64_t lim = (int64_t)1 << 30;
  return ld_x >= H && ld_x <= lim && n_src >= 1 && n_src <= lim && (row_index != nullptr || n_src >= N) && tmi_aligned(row_index, 4);
}
drop_t ch_drop_of(float p, uint64_t seed) {
  drop_t d;
  d.on = p > 0.f;
  d.key = tmi_stream_key(seed, 0);
  d.thr = tmi_drop_thr(p);
  d.scale = tmi_keep_scale(d.thr);
  return d;
}
inline bool f4(const void* p) { return p != nullptr && tmi_aligned(p, 4); }
inline bool f4n(const void* p) { return tmi_aligned(p, 4); }  // (may be NULL)

}  // namespace

extern "C" int64_t tmi_cls_head_workspace_bytes(int64_t N, int64_t H, int64_t P, int64_t C) {
  if (!ch_sizes_ok(N, H, P, C)) return -1;
  return CH_HDR + (N * P + ch_part_floats(N, H, P, C)) * 4;
}

static int tmi_cls_head_fwd_impl(const float* pooled, int64_t ld_x, int64_t n_src, const int32_t* row_index, const float* Wp,
                                 const float* bp, const float* Wc, const float* bc, const int32_t* labels, float p, uint64_t seed,
                                 float* logits, int64_t ld_logits, int32_t* pred, float* z, int64_t ld_z, float* log_probs,
                                 int64_t ld_lp, float* nll, int32_t* label_rank, int64_t* confusion, int64_t ld_conf, int64_t N,
                                 int64_t H, int64_t P, int64_t C, void* stream) {
  const int64_t lim = (int64_t)1 << 30;
  const bool ok = ch_sizes_ok(N, H, P, C) && ch_p_ok(p) && ch_rows_ok(ld_x, n_src, row_index, N, H) && f4(pooled) && f4(Wp) &&
                  f4(bp) && f4(Wc) && f4(bc) && f4n(labels) && f4(logits) && f4(pred) && f4n(z) && f4n(log_probs) && f4n(nll) &&
                  f4n(label_rank) && tmi_aligned(confusion, 8) && ld_logits >= C && ld_logits <= lim &&
                  (z == nullptr || (ld_z >= P && ld_z <= lim)) && (log_probs == nullptr || (ld_lp >= C && ld_lp <= lim)) &&
                  (confusion == nullptr || (ld_conf >= C && ld_conf <= lim));
  if (!ok) {
    tmi_set_error("tmi_cls_head_fwd: bad argument (1 <= N <= 65535; H <= 4096, a multiple of 4; P even, <= 1024; 1 <= C <= 1024; "
                  "0 <= p < 1; ld_x >= H, ld_logits >= C, ld_z >= P, ld_lp >= C, ld_conf >= C, all <= 2^30; n_src >= 1, and >= N "
                  "without a row_index; pooled, Wp, bp, Wc, bc, logits, pred non-NULL; pointers 4-byte aligned, confusion 8)");
    return TMI_ERR_INVALID;
  }
  const int LS = C > CH_HC ? (int)C : CH_HC;
  const size_t lds = (size_t)CH_TR * (size_t)(P + LS) * sizeof(float);  // <= 8 * 2048 * 4 = 64 KB
  hipLaunchKernelGGL(cls_fwd_kernel, dim3((unsigned)((N + CH_TR - 1) / CH_TR)), dim3(CH_THREADS), lds,
                     reinterpret_cast<hipStream_t>(stream), pooled, ld_x, n_src, row_index, Wp, bp, Wc, bc, labels,
                     ch_drop_of(p, seed), logits, ld_logits, pred, z, ld_z, log_probs, ld_lp, nll, label_rank,
                     reinterpret_cast<unsigned long long*>(confusion), ld_conf, (int)N, (int)H, (int)P, (int)C);
  return tmi_check_launch("tmi_cls_head_fwd");
}

extern "C" int tmi_cls_head_fwd(const float* pooled, int64_t ld_x, int64_t n_src, const int32_t* row_index, const float* Wp,
                                const float* bp, const float* Wc, const float* bc, const int32_t* labels, float p, uint64_t seed,
                                float* logits, int64_t ld_logits, int32_t* pred, float* z, int64_t ld_z, float* log_probs,
                                int64_t ld_lp, float* nll, int32_t* label_rank, int64_t* confusion, int64_t ld_conf, int64_t N,
                                int64_t H, int64_t P, int64_t C, void* stream) {
  return tmi_plan_run<tmi_cls_head_fwd_impl>(pooled, ld_x, n_src, row_index, Wp, bp, Wc, bc, labels, p, tmi_plan_seed{seed}, logits,
                                             ld_logits, pred, z, ld_z, log_probs, ld_lp, nll, label_rank, confusion, ld_conf, N, H,
                                             P, C, stream);
}

static int tmi_cls_head_bwd_impl(const float* pooled, int64_t ld_x, int64_t n_src, const int32_t* row_index, const float* Wc,
                                 const int32_t* labels, float p, uint64_t seed, const float* z, int64_t ld_z,
                                 const float* log_probs, int64_t ld_lp, float* gWp, float* gbp, float* gWc, float* gbc, float* loss,
                                 void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t P, int64_t C,
                                 void* stream) {
  const int64_t lim = (int64_t)1 << 30;
  const bool ok = ch_sizes_ok(N, H, P, C) && ch_p_ok(p) && ch_rows_ok(ld_x, n_src, row_index, N, H) && f4(pooled) && f4(Wc) &&
                  f4(labels) && f4(z) && f4(log_probs) && f4(gWp) && f4(gbp) && f4(gWc) && f4(gbc) && f4(loss) &&
                  workspace != nullptr && tmi_aligned(workspace, 16) && workspace_bytes >= CH_HDR + (N * P + ch_part_floats(N, H, P, C)) * 4 && ld_z >= P &&
                  ld_z <= lim && ld_lp >= C && ld_lp <= lim;
  if (!ok) {
    tmi_set_error("tmi_cls_head_bwd: bad argument (the sizes, p and strides of tmi_cls_head_fwd; every pointer but row_index "
                  "non-NULL and 4-byte aligned; workspace 16-byte aligned, of tmi_cls_head_workspace_bytes(N, H, P, C) bytes)");
    return TMI_ERR_INVALID;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  int32_t* hdr = reinterpret_cast<int32_t*>(workspace);
  float* dpre = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + CH_HDR);
  const drop_t drop = ch_drop_of(p, seed);
  hipLaunchKernelGGL(cls_count_kernel, dim3(1), dim3(CH_THREADS), 0, st, labels, log_probs, ld_lp, (int)N, (int)C, hdr, loss);
  int rc = tmi_check_launch("tmi_cls_head_bwd");
  if (rc != 0) return rc;
  hipLaunchKernelGGL(cls_dpre_kernel, dim3((unsigned)((N + CH_TR - 1) / CH_TR)), dim3(CH_THREADS),
                     (size_t)CH_TR * (size_t)C * sizeof(float), st, Wc, labels, drop, z, ld_z, log_probs, ld_lp, hdr, dpre, (int)N,
                     (int)P, (int)C);
  rc = tmi_check_launch("tmi_cls_head_bwd");
  if (rc != 0) return rc;
  const unsigned nchunk = (unsigned)((N + CO_CR - 1) / CO_CR);
  float* part = nchunk > 1 ? dpre + N * P : nullptr;  // (the two products run one after the other and share it)
  hipLaunchKernelGGL(cls_outer_kernel<0>, dim3((unsigned)((P + CO_T - 1) / CO_T), (unsigned)((C + CO_T - 1) / CO_T), nchunk),
                     dim3(CH_THREADS), 0, st, pooled, ld_x, n_src, row_index, labels, drop, z, ld_z, log_probs, ld_lp, hdr, dpre,
                     gWc, gbc, part, (int)N, (int)P, (int)C, (int)P);
  rc = tmi_check_launch("tmi_cls_head_bwd");
  if (rc != 0) return rc;
  if (part != nullptr) {
    hipLaunchKernelGGL(cls_fold_kernel, dim3((unsigned)((P * C + C + CH_THREADS - 1) / CH_THREADS)), dim3(CH_THREADS), 0, st, part,
                       (int)nchunk, P * C, C, gWc, gbc);
    rc = tmi_check_launch("tmi_cls_head_bwd");
    if (rc != 0) return rc;
  }
  hipLaunchKernelGGL(cls_outer_kernel<1>, dim3((unsigned)((H + CO_T - 1) / CO_T), (unsigned)((P + CO_T - 1) / CO_T), nchunk),
                     dim3(CH_THREADS), 0, st, pooled, ld_x, n_src, row_index, labels, drop, z, ld_z, log_probs, ld_lp, hdr, dpre,
                     gWp, gbp, part, (int)N, (int)H, (int)P, (int)P);
  rc = tmi_check_launch("tmi_cls_head_bwd");
  if (rc != 0 || part == nullptr) return rc;
  hipLaunchKernelGGL(cls_fold_kernel, dim3((unsigned)((H * P + P + CH_THREADS - 1) / CH_THREADS)), dim3(CH_THREADS), 0, st, part,
                     (int)nchunk, H * P, P, gWp, gbp);
  return tmi_check_launch("tmi_cls_head_bwd");
}

extern "C" int tmi_cls_head_bwd(const float* pooled, int64_t ld_x, int64_t n_src, const int32_t* row_index, const float* Wc,
                                const int32_t* labels, float p, uint64_t seed, const float* z, int64_t ld_z,
                                const float* log_probs, int64_t ld_lp, float* gWp, float* gbp, float* gWc, float* gbc, float* loss,
                                void* workspace, int64_t workspace_bytes, int64_t N, int64_t H, int64_t P, int64_t C,
                                void* stream) {
  return tmi_plan_run<tmi_cls_head_bwd_impl>(pooled, ld_x, n_src, row_index, Wc, labels, p, tmi_plan_seed{seed}, z, ld_z, log_probs,
                                             ld_lp, gWp, gbp, gWc, gbc, loss, workspace, workspace_bytes, N, H, P, C, stream);
}
