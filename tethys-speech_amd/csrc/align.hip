// Token-to-frame alignment (inference): tmi_align_cost and tmi_dtw.  include/tethys_mi.h states both contracts; this is
// how they are carried out.
//
// tmi_align_cost - cross-attention weights [N, H, S, T] of one decoder layer -> the DTW cost [N, S, T].
//   One workgroup of sixteen waves per (item, frame tile).  The 64 lanes of a wave lie along the frames, so every load of a
//   row is one contiguous piece; a tile is AC_LANES - (w - 1) output frames and the w/2 halo frames on either side of it are
//   simply the outermost lanes.  A lane past an end of the valid range [0, cols) loads the REFLECTED frame (-k -> k,
//   cols-1+k -> cols-1-k) and runs the same arithmetic on it as the lane that owns that frame, so the halo values are the
//   owner's bit for bit and the median window of output lane l is the values of lanes l - w/2 .. l + w/2: w lane shuffles,
//   no LDS image of the tile.  Wave v takes the rows s = v, v + 16, ...
//   Per head with a non-zero weight (a zero-weight head is never loaded):
//     mean  = ((a0 + a1) + ... + a15) / rows        a_v: wave v's sum of its rows in ascending s        (fp32)
//     var   = ((b0 + b1) + ... + b15) / rows        b_v: wave v's fma chain of (p - mean)^2             (two-pass)
//     rstd  = rsqrtf(var + 1e-20f)
//   both kept in LDS per (head, lane).  Then, per row, acc = accumulate ? cost : 0 and for h ascending
//     z = (p - mean) * rstd (or p), m = median of the window (a min / max selection network: it selects, it does not
//     round), acc = fmaf(-weight[h], m, acc);
//   one store of acc.  The weights are read three times (sum, squares, filter) - the second and third time from L2, a
//   tile of one head is 448 x 64 x 4 bytes at most - and the cost is written once.  No atomics; every order is fixed.
//
// tmi_dtw - one workgroup per item, one thread per row, the anti-diagonal wavefront: at step d thread i owns cell
//   (i, d - i).  A thread keeps its own last value (the left neighbour D[i][j-1]) and the last two values of the thread
//   above (D[i-1][j], D[i-1][j-1]) in registers; the upper thread's last value arrives by a lane shuffle inside a wave and
//   through a two-slot LDS word per wave across a wave boundary (slot d & 1, so ONE barrier per diagonal orders both the
//   read of the previous step's slot and the write of this step's).  The costs of the next DT_PF steps are loaded while
//   the current DT_PF are computed (a thread walks along its own row: neighbouring lanes are on different cache lines, so
//   the latency has to be covered, not the bandwidth).  Moves are packed 2 bits per cell, one 32-bit word per 16 columns
//   of a row, into the workspace [N][S_max][ceil(T_max / 16)]; after the last diagonal thread 0 walks back from
//   (rows-1, cols-1) through move words that the whole workgroup stages in LDS a piece of rows at a time, and leaves the
//   path (reversed) and the token bounds in LDS, from where the workgroup copies them out.  Measured
//   (profiles/r15_align.json): about 0.45 us per diagonal, the same with the walk on global memory and with a barrier
//   that waits for LDS only - what a diagonal costs is not yet accounted for.  Same inputs, same bits: no atomics, one fixed order.
#include "tmi_common.h"
#include <math.h>

namespace {

constexpr int AC_THREADS = 1024;  // 16 waves: the kernel waits on loads; with 4 waves it took 3x as long (profiles/r15_align.json has the 16-wave figures)
constexpr int AC_WAVES = AC_THREADS / TMI_WAVE;
constexpr int AC_LANES = 64;   // frames a tile loads: its outputs and the halo
constexpr int AC_HMAX = 32;    // heads per call
constexpr int AC_WMAX = 9;     // widest median window

constexpr int DT_SMAX = 1024;  // rows: one thread each
constexpr int DT_TMAX = 4096;  // columns: the path (<= DT_SMAX + DT_TMAX - 1 cells) is staged in LDS
constexpr int DT_PF = 8;       // diagonals per cost prefetch
constexpr int DT_CHUNK = 8192; // move words staged in LDS per piece of the walk back (>= 32 rows at DT_TMAX)

__device__ __forceinline__ void cx(float& a, float& b) {  // a <- min, b <- max
  const float lo = fminf(a, b), hi = fmaxf(a, b);
  a = lo, b = hi;
}

// median of the W values held by lanes lane - W/2 .. lane + W/2 (a lane outside the wave wraps: its result is not used)
template <int W> __device__ __forceinline__ float window_median(float z, int lane) {
  if constexpr (W == 1) {
    return z;
  } else {
    float p[W];
#pragma unroll
    for (int k = 0; k < W; ++k) p[k] = __shfl(z, (lane + k - W / 2) & 63, 64);
    if constexpr (W == 3) {
      return __builtin_amdgcn_fmed3f(p[0], p[1], p[2]);
    } else if constexpr (W == 5) {
      // drop the smallest and the largest of the first four, then the middle of what is left and the fifth
      const float f = fmaxf(fminf(p[0], p[1]), fminf(p[2], p[3]));
      const float g = fminf(fmaxf(p[0], p[1]), fmaxf(p[2], p[3]));
      return __builtin_amdgcn_fmed3f(p[4], f, g);
    } else if constexpr (W == 7) {  // 13 exchanges
      cx(p[0], p[5]); cx(p[0], p[3]); cx(p[1], p[6]); cx(p[2], p[4]); cx(p[0], p[1]); cx(p[3], p[5]); cx(p[2], p[6]);
      cx(p[2], p[3]); cx(p[3], p[6]); cx(p[4], p[5]); cx(p[1], p[4]); cx(p[1], p[3]); cx(p[3], p[4]);
      return p[3];
    } else {  // W == 9: 19 exchanges
      cx(p[1], p[2]); cx(p[4], p[5]); cx(p[7], p[8]); cx(p[0], p[1]); cx(p[3], p[4]); cx(p[6], p[7]); cx(p[1], p[2]);
      cx(p[4], p[5]); cx(p[7], p[8]); cx(p[0], p[3]); cx(p[5], p[8]); cx(p[4], p[7]); cx(p[3], p[6]); cx(p[1], p[4]);
      cx(p[2], p[5]); cx(p[4], p[7]); cx(p[4], p[2]); cx(p[6], p[4]); cx(p[4], p[2]);
      return p[4];
    }
  }
}

// the AC_WAVES partial sums of a frame, wave 0's first
__device__ __forceinline__ float fold_waves(const float (*red)[AC_LANES], int lane) {
  float a = red[0][lane];
#pragma unroll
  for (int v = 1; v < AC_WAVES; ++v) a += red[v][lane];
  return a;
}

template <typename T, int W>
__global__ __launch_bounds__(AC_THREADS) void align_cost_kernel(
    const T* __restrict__ probs, int64_t p_sbh, int64_t p_sq, const int32_t* __restrict__ rows_p,
    const int32_t* __restrict__ cols_p, const float* __restrict__ head_weight, float* __restrict__ cost, int64_t c_sn,
    int64_t c_ss, int H, int S, int Tn, int normalize, int accumulate) {
  constexpr int HW = W / 2, TILE = AC_LANES - 2 * HW;
  __shared__ float s_mean[AC_HMAX][AC_LANES], s_rstd[AC_HMAX][AC_LANES], s_red[AC_WAVES][AC_LANES], s_w[AC_HMAX];
  const int n = blockIdx.y;
  int rows = rows_p[n], cols = cols_p[n];
  rows = rows > S ? S : rows;  // (a value outside the contract never leads outside the tensors)
  cols = cols > Tn ? Tn : cols;
  const int c0 = blockIdx.x * TILE;
  if (rows < 1 || cols <= HW || c0 >= cols) return;  // (uniform over the workgroup)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int j = c0 - HW + lane;  // the frame this lane holds
  j = j < 0 ? -j : j;
  j = j > cols - 1 ? 2 * (cols - 1) - j : j;
  j = j < 0 ? 0 : (j > cols - 1 ? cols - 1 : j);  // (lanes past the last halo frame: loaded, never used)
  const int t = c0 + lane - HW;
  const bool out = lane >= HW && lane < AC_LANES - HW && t < cols;
  const T* __restrict__ pn = probs + (int64_t)n * H * p_sbh + j;
  if (threadIdx.x < H) s_w[threadIdx.x] = head_weight[threadIdx.x];
  __syncthreads();

  if (normalize) {
    const float nrows = (float)rows;
    for (int h = 0; h < H; ++h) {
      if (s_w[h] == 0.f) continue;  // (uniform)
      const T* __restrict__ ph = pn + (int64_t)h * p_sbh;
      float a = 0.f;
      for (int s = wv; s < rows; s += AC_WAVES) a += to_f32(ph[(int64_t)s * p_sq]);
      s_red[wv][lane] = a;
      __syncthreads();
      const float mean = fold_waves(s_red, lane) / nrows;
      __syncthreads();
      float b = 0.f;
      for (int s = wv; s < rows; s += AC_WAVES) {
        const float dlt = to_f32(ph[(int64_t)s * p_sq]) - mean;
        b = fmaf(dlt, dlt, b);
      }
      s_red[wv][lane] = b;
      __syncthreads();
      const float var = fold_waves(s_red, lane) / nrows;
      if (wv == 0) {
        s_mean[h][lane] = mean;
        s_rstd[h][lane] = rsqrtf(var + 1e-20f);
      }
      __syncthreads();
    }
  }

  float* __restrict__ cn = cost + (int64_t)n * c_sn + (out ? t : 0);
  for (int s = wv; s < rows; s += AC_WAVES) {  // (uniform over the wave: the shuffles see all 64 lanes)
    float acc = (accumulate && out) ? cn[(int64_t)s * c_ss] : 0.f;
    for (int h = 0; h < H; ++h) {
      const float wgt = s_w[h];
      if (wgt == 0.f) continue;
      float z = to_f32(pn[(int64_t)h * p_sbh + (int64_t)s * p_sq]);
      if (normalize) z = (z - s_mean[h][lane]) * s_rstd[h][lane];
      acc = fmaf(-wgt, window_median<W>(z, lane), acc);
    }
    if (out) cn[(int64_t)s * c_ss] = acc;
  }
}

template <typename T, int W>
void align_cost_launch(const void* probs, int64_t p_sbh, int64_t p_sq, const int32_t* rows, const int32_t* cols,
                       const float* head_weight, float* cost, int64_t c_sn, int64_t c_ss, int64_t N, int64_t H, int64_t S,
                       int64_t Tn, int normalize, int accumulate, hipStream_t s) {
  constexpr int TILE = AC_LANES - 2 * (W / 2);
  const dim3 grid((unsigned)((Tn + TILE - 1) / TILE), (unsigned)N);
  hipLaunchKernelGGL((align_cost_kernel<T, W>), grid, dim3(AC_THREADS), 0, s, reinterpret_cast<const T*>(probs), p_sbh, p_sq,
                     rows, cols, head_weight, cost, c_sn, c_ss, (int)H, (int)S, (int)Tn, normalize, accumulate);
}

template <typename T>
void align_cost_width(int W, const void* probs, int64_t p_sbh, int64_t p_sq, const int32_t* rows, const int32_t* cols,
                      const float* hw, float* cost, int64_t c_sn, int64_t c_ss, int64_t N, int64_t H, int64_t S, int64_t Tn,
                      int normalize, int accumulate, hipStream_t s) {
  switch (W) {
    case 1: align_cost_launch<T, 1>(probs, p_sbh, p_sq, rows, cols, hw, cost, c_sn, c_ss, N, H, S, Tn, normalize, accumulate, s); break;
    case 3: align_cost_launch<T, 3>(probs, p_sbh, p_sq, rows, cols, hw, cost, c_sn, c_ss, N, H, S, Tn, normalize, accumulate, s); break;
    case 5: align_cost_launch<T, 5>(probs, p_sbh, p_sq, rows, cols, hw, cost, c_sn, c_ss, N, H, S, Tn, normalize, accumulate, s); break;
    case 7: align_cost_launch<T, 7>(probs, p_sbh, p_sq, rows, cols, hw, cost, c_sn, c_ss, N, H, S, Tn, normalize, accumulate, s); break;
    default: align_cost_launch<T, 9>(probs, p_sbh, p_sq, rows, cols, hw, cost, c_sn, c_ss, N, H, S, Tn, normalize, accumulate, s); break;
  }
}

// ------------------------------------------------------------------------------------------------------------ the warp
__device__ __forceinline__ uint32_t dt_step(float c, float c0, float c1, float c2, float& own) {
  uint32_t mv;
  if (c0 < c1 && c0 < c2) mv = 0u;
  else if (c1 < c0 && c1 < c2) mv = 1u;
  else mv = 2u;
  own = c + fminf(c0, fminf(c1, c2));
  return mv;
}

__global__ __launch_bounds__(DT_SMAX) void dtw_kernel(const float* __restrict__ cost, int64_t c_sn, int64_t c_ss,
                                                      const int32_t* __restrict__ rows_p, const int32_t* __restrict__ cols_p,
                                                      int S_max, int T_max, int32_t* __restrict__ tok_start,
                                                      int32_t* __restrict__ tok_end, float* __restrict__ total,
                                                      int32_t* __restrict__ path, int32_t* __restrict__ path_len,
                                                      uint32_t* moves_ws) {
  __shared__ float s_bnd[2][DT_SMAX / TMI_WAVE];
  __shared__ int32_t s_tok[2][DT_SMAX];
  __shared__ uint32_t s_path[DT_SMAX + DT_TMAX - 1];  // (i << 16 | j), last cell first
  __shared__ uint32_t s_mv[DT_CHUNK];
  __shared__ int s_pos[4];  // the walk's row, column, path length so far, done
  const int n = blockIdx.x;
  int rows = rows_p[n], cols = cols_p[n];
  rows = rows > S_max ? S_max : rows;
  cols = cols > T_max ? T_max : cols;
  if (rows < 1 || cols < 1) return;  // (uniform: outside the contract, nothing is written)
  const int i = threadIdx.x, lane = i & 63, wv = i >> 6;
  const int wpr = (T_max + 15) >> 4;  // move words per row
  const float* __restrict__ ci = cost + (int64_t)n * c_sn + (int64_t)(i < rows ? i : 0) * c_ss;
  uint32_t* mi = moves_ws + ((int64_t)n * S_max + (i < rows ? i : 0)) * wpr;
  if (i < 2 * (DT_SMAX / TMI_WAVE)) (&s_bnd[0][0])[i] = INFINITY;
  __syncthreads();

  float own = INFINITY;               // D[i][j-1]; D[i][cols-1] once the row is done
  float up2 = i == 0 ? 0.f : INFINITY;  // D[i-1][j-1]
  uint32_t word = 0u;
  const int nsteps = rows + cols - 1;
  float cur[DT_PF], nxt[DT_PF];
#pragma unroll
  for (int k = 0; k < DT_PF; ++k) {
    const int j = k - i;
    cur[k] = (i < rows && j >= 0 && j < cols) ? ci[j] : 0.f;
  }
  for (int d0 = 0; d0 < nsteps; d0 += DT_PF) {  // (every thread runs every step: the barriers and shuffles are uniform)
#pragma unroll
    for (int k = 0; k < DT_PF; ++k) {
      const int j = d0 + DT_PF + k - i;
      nxt[k] = (i < rows && j >= 0 && j < cols) ? ci[j] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < DT_PF; ++k) {
      const int d = d0 + k, j = d - i;
      float up1 = __shfl_up(own, 1, 64);  // D[i-1][j]: the upper thread's value of step d - 1
      if (lane == 0) up1 = wv > 0 ? s_bnd[(d + 1) & 1][wv - 1] : INFINITY;
      if (i < rows && j >= 0 && j < cols) {
        const uint32_t mv = dt_step(cur[k], up2, up1, own, own);
        word |= mv << (2 * (j & 15));
        if ((j & 15) == 15 || j == cols - 1) {
          mi[j >> 4] = word;
          word = 0u;
        }
      }
      up2 = up1;
      if (lane == 63) s_bnd[d & 1][wv] = own;
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < DT_PF; ++k) cur[k] = nxt[k];
  }
  if (i == rows - 1) total[n] = own;
  __threadfence_block();  // the move words of every row, before thread 0 reads them
  __syncthreads();

  // The walk back, a piece of rows at a time: the whole workgroup stages the move words of the next `ch` rows (columns
  // up to the current one) in LDS, then thread 0 walks through them.
  const int ch = DT_CHUNK / wpr;
  if (i == 0) {
    s_pos[0] = rows - 1, s_pos[1] = cols - 1, s_pos[2] = 0, s_pos[3] = 0;
    s_tok[1][rows - 1] = cols;
  }
  __syncthreads();
  for (;;) {
    const int r_hi = s_pos[0], c_hi = s_pos[1];  // (uniform: written before the barrier that ends the previous piece)
    if (s_pos[3]) break;
    const int r_lo = r_hi - ch + 1 > 0 ? r_hi - ch + 1 : 0;
    const int nw = (c_hi >> 4) + 1;
    for (int k = i; k < (r_hi - r_lo + 1) * nw; k += blockDim.x) {
      const int rr = k / nw, ww = k - rr * nw;
      s_mv[rr * wpr + ww] = moves_ws[((int64_t)n * S_max + r_lo + rr) * wpr + ww];
    }
    __syncthreads();
    if (i == 0) {
      int r = r_hi, c = c_hi, len = s_pos[2];
      bool done = false;
      while (r >= r_lo) {
        s_path[len++] = ((uint32_t)r << 16) | (uint32_t)c;
        if (r == 0 && c == 0) {
          done = true;
          break;
        }
        uint32_t mv = (s_mv[(r - r_lo) * wpr + (c >> 4)] >> (2 * (c & 15))) & 3u;
        if (r == 0) mv = 2u;       // (what the recurrence gives for finite costs; also keeps the walk inside the matrix
        else if (c == 0) mv = 1u;  //  when the costs are not finite)
        if (mv == 2u) {
          --c;
        } else {
          s_tok[0][r] = c;
          --r;
          if (mv == 0u) --c;
          s_tok[1][r] = c + 1;
        }
      }
      if (done) s_tok[0][0] = 0;
      s_pos[0] = r, s_pos[1] = c, s_pos[2] = len, s_pos[3] = done ? 1 : 0;
    }
    __syncthreads();
  }
  const int len = s_pos[2];
  if (i < rows) {
    tok_start[(int64_t)n * S_max + i] = s_tok[0][i];
    tok_end[(int64_t)n * S_max + i] = s_tok[1][i];
  }
  if (path != nullptr) {
    int32_t* __restrict__ pn = path + (int64_t)n * (S_max + T_max - 1) * 2;
    for (int k = i; k < len; k += blockDim.x) {
      const uint32_t v = s_path[len - 1 - k];
      pn[2 * k] = (int32_t)(v >> 16);
      pn[2 * k + 1] = (int32_t)(v & 0xffffu);
    }
    if (i == 0) path_len[n] = len;
  }
}

}  // namespace

extern "C" int64_t tmi_align_cost_tile(int32_t medfilt_width) {
  if (medfilt_width < 1 || medfilt_width > AC_WMAX || !(medfilt_width & 1)) return -1;
  return AC_LANES - 2 * (medfilt_width / 2);
}

static int tmi_align_cost_impl(const void* probs, int32_t probs_dtype, int64_t p_sbh, int64_t p_sq, const int32_t* rows,
                               const int32_t* cols, const float* head_weight, float* cost, int64_t c_sn, int64_t c_ss,
                               int64_t N, int64_t H, int64_t S, int64_t T, int32_t medfilt_width, int32_t normalize,
                               int32_t accumulate, void* stream) {
  const bool dt_ok = probs_dtype == TMI_F32 || probs_dtype == TMI_BF16;
  const int64_t lim = (int64_t)1 << 30;
  if (!probs || !rows || !cols || !head_weight || !cost || !dt_ok || !tmi_aligned(probs, probs_dtype == TMI_BF16 ? 2 : 4) ||
      !tmi_aligned(rows, 4) || !tmi_aligned(cols, 4) || !tmi_aligned(head_weight, 4) || !tmi_aligned(cost, 4) || N < 1 || N > 65535 || H < 1 ||
      H > AC_HMAX || S < 1 || S > lim || T < 1 || T > lim || medfilt_width < 1 || medfilt_width > AC_WMAX ||
      !(medfilt_width & 1) || T <= medfilt_width / 2 || p_sq < T || p_sq > lim || p_sbh < S * p_sq || c_ss < T || c_ss > lim ||
      c_sn < S * c_ss || (normalize != 0 && normalize != 1) || (accumulate != 0 && accumulate != 1)) {
    tmi_set_error("tmi_align_cost: bad argument (non-NULL pointers; dtype fp32 / bf16; 1 <= N <= 65535, 1 <= H <= 32; "
                  "medfilt_width odd in 1..9, medfilt_width / 2 < T; p_sq >= T, p_sbh >= S p_sq, c_ss >= T, c_sn >= S c_ss; flags 0 / 1)");
    return TMI_ERR_INVALID;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (probs_dtype == TMI_BF16)
    align_cost_width<bf16_t>(medfilt_width, probs, p_sbh, p_sq, rows, cols, head_weight, cost, c_sn, c_ss, N, H, S, T, normalize,
                             accumulate, s);
  else
    align_cost_width<float>(medfilt_width, probs, p_sbh, p_sq, rows, cols, head_weight, cost, c_sn, c_ss, N, H, S, T, normalize,
                            accumulate, s);
  return tmi_check_launch("tmi_align_cost");
}

extern "C" int tmi_align_cost(const void* probs, int32_t probs_dtype, int64_t p_sbh, int64_t p_sq, const int32_t* rows,
                              const int32_t* cols, const float* head_weight, float* cost, int64_t c_sn, int64_t c_ss, int64_t N,
                              int64_t H, int64_t S, int64_t T, int32_t medfilt_width, int32_t normalize, int32_t accumulate,
                              void* stream) {
  return tmi_plan_run<tmi_align_cost_impl>(probs, probs_dtype, p_sbh, p_sq, rows, cols, head_weight, cost, c_sn, c_ss, N, H, S, T,
                                           medfilt_width, normalize, accumulate, stream);
}

extern "C" int64_t tmi_dtw_workspace_bytes(int64_t N, int64_t S_max, int64_t T_max) {
  if (N < 1 || N > 65535 || S_max < 1 || S_max > DT_SMAX || T_max < 1 || T_max > DT_TMAX) return -1;
  return N * S_max * ((T_max + 15) / 16) * (int64_t)sizeof(uint32_t);
}

static int tmi_dtw_impl(const float* cost, int64_t c_sn, int64_t c_ss, const int32_t* rows, const int32_t* cols, int64_t N,
                        int64_t S_max, int64_t T_max, int32_t* tok_start, int32_t* tok_end, float* total, int32_t* path,
                        int32_t* path_len, void* workspace, int64_t workspace_bytes, void* stream) {
  const int64_t need = tmi_dtw_workspace_bytes(N, S_max, T_max);
  if (!cost || !rows || !cols || !tok_start || !tok_end || !total || !workspace || (path != nullptr) != (path_len != nullptr) ||
      !tmi_aligned(cost, 4) || !tmi_aligned(rows, 4) || !tmi_aligned(cols, 4) || !tmi_aligned(tok_start, 4) || !tmi_aligned(tok_end, 4) || !tmi_aligned(total, 4) ||
      !tmi_aligned(path, 4) || !tmi_aligned(path_len, 4) || !tmi_aligned(workspace, 4) || need < 0 || workspace_bytes < need || c_ss < T_max ||
      c_ss > ((int64_t)1 << 30) || c_sn < S_max * c_ss) {
    tmi_set_error("tmi_dtw: bad argument (non-NULL pointers, path and path_len together; 1 <= N <= 65535, 1 <= S_max <= 1024 "
                  "rows, 1 <= T_max <= 4096 columns; c_ss >= T_max, c_sn >= S_max c_ss; workspace of tmi_dtw_workspace_bytes)");
    return TMI_ERR_INVALID;
  }
  const unsigned threads = (unsigned)((S_max + TMI_WAVE - 1) / TMI_WAVE * TMI_WAVE);
  hipLaunchKernelGGL(dtw_kernel, dim3((unsigned)N), dim3(threads), 0, reinterpret_cast<hipStream_t>(stream), cost, c_sn, c_ss,
                     rows, cols, (int)S_max, (int)T_max, tok_start, tok_end, total, path, path_len,
                     reinterpret_cast<uint32_t*>(workspace));
  return tmi_check_launch("tmi_dtw");
}

extern "C" int tmi_dtw(const float* cost, int64_t c_sn, int64_t c_ss, const int32_t* rows, const int32_t* cols, int64_t N,
                       int64_t S_max, int64_t T_max, int32_t* tok_start, int32_t* tok_end, float* total, int32_t* path,
                       int32_t* path_len, void* workspace, int64_t workspace_bytes, void* stream) {
  return tmi_plan_run<tmi_dtw_impl>(cost, c_sn, c_ss, rows, cols, N, S_max, T_max, tok_start, tok_end, total, path, path_len,
                                    workspace, workspace_bytes, stream);
}
