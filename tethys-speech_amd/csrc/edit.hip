// Error-rate evaluation: tmi_edit_distance.  include/tethys_mi.h states the rule; this is how it is carried out.
//
// One workgroup per (hypothesis, reference) pair.
//   Normalisation.  Each row is compacted into LDS by the whole workgroup.  First the cut: every thread looks at its
//   positions p = tid, tid + threads, .. below min(len, cols) for stop_id, the smallest such p of a wave is found by a
//   butterfly of lane shuffles and the smallest over the waves through one LDS word per wave.  Then, a piece of `threads`
//   positions at a time, a ballot over the keep flags gives a lane its rank inside the wave (popcount of the lower
//   lanes' bits) and the wave its count; the counts of the waves before it and the pieces before this one are added to
//   it, so the kept tokens land in LDS in their order.  A token is only compared (with stop_id, the skip bounds and,
//   later, the other row's tokens), never used as an index.
//   The table.  Anti-diagonal k holds the cells (i, j) with i + j = k, stored at index j of one of three rotating LDS
//   diagonals (k mod 3); cell (i, j) reads (i-1, j-1) from diagonal k - 2 and (i-1, j), (i, j-1) from diagonal k - 1,
//   and the borders i == 0 / j == 0 are written from their closed form.  The threads take the cells of a diagonal in
//   ascending j, `threads` apart; ONE barrier per diagonal orders the writes of diagonal k before the reads of k + 1
//   and the reads of diagonal k - 2 before diagonal k + 1 overwrites it.  A cell is one 64-bit word of four 14-bit
//   fields (d, sub, del, ins <= 8192); a candidate is the neighbour's word plus a constant, and candidates are compared
//   by the d field alone, in the order diagonal, up, left, a later one winning only when strictly smaller.
//   A pair with an empty side is written from the closed form without a sweep.  Thread 0 writes the six outputs.
// The workgroup is as many waves as the reference has columns (64 .. 1024 threads), so a reference of up to 64 columns
// runs on one wave, where the barrier costs nothing; the LDS is sized by the call's columns
// (3 (ref_cols + 1) 8 + (hyp_cols + ref_cols) 4 bytes, 131096 at the limits).  No atomics; every order is fixed.
#include "tmi_common.h"

namespace {

constexpr int ED_MAXC = 4096;     // columns read of either side
constexpr int ED_THREADS = 1024;  // the largest workgroup
constexpr int ED_WAVES = ED_THREADS / TMI_WAVE;
constexpr uint64_t ED_D = 0x3fffull;  // the d field
constexpr uint64_t ED_SUB = 1ull | (1ull << 14), ED_DEL = 1ull | (1ull << 28), ED_INS = 1ull | (1ull << 42);

constexpr int64_t ed_lds_bytes(int64_t hyp_cols, int64_t ref_cols) {
  return 3 * (ref_cols + 1) * 8 + (hyp_cols + ref_cols) * 4;
}

// the kept tokens of `row` -> dst[0 .. count), in order; returns the count (the same in every thread).  Every thread of
// the workgroup calls it; s_w is ED_WAVES words of LDS.  Ends on a barrier.
__device__ int ed_compact(const int32_t* __restrict__ row, int len, int32_t stop_id, int32_t skip_lo, int32_t skip_hi,
                          int32_t* dst, int* s_w) {
  const int tid = threadIdx.x, T = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = T >> 6;
  int cut = len;
  if (stop_id != -1) {
    for (int p = tid; p < len; p += T)
      if (row[p] == stop_id) {
        cut = p;
        break;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(cut, o, 64);
      cut = other < cut ? other : cut;
    }
    if (lane == 0) s_w[wv] = cut;
    __syncthreads();
    for (int w = 0; w < nw; ++w) cut = s_w[w] < cut ? s_w[w] : cut;
    __syncthreads();
  }
  int base = 0;
  for (int p0 = 0; p0 < cut; p0 += T) {  // (uniform: cut is the same in every thread)
    const int p = p0 + tid;
    const int32_t x = p < cut ? row[p] : 0;
    const bool keep = p < cut && !(x >= skip_lo && x < skip_hi);
    const unsigned long long bal = __ballot(keep);
    if (lane == 0) s_w[wv] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int w = 0; w < nw; ++w) {
      const int c = s_w[w];
      off += w < wv ? c : 0;
      base += c;
    }
    if (keep) dst[off + __popcll(bal & ((1ull << lane) - 1ull))] = x;
    __syncthreads();
  }
  return base;
}

__global__ __launch_bounds__(ED_THREADS) void edit_distance_kernel(
    const int32_t* __restrict__ hyp, int64_t hyp_ld, int hyp_cols, const int32_t* __restrict__ hyp_len,
    const int32_t* __restrict__ ref, int64_t ref_ld, int ref_cols, const int32_t* __restrict__ ref_len, int R,
    int32_t stop_id, int32_t skip_lo, int32_t skip_hi, int32_t* __restrict__ out, int64_t out_ld) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_w[ED_WAVES];
  const int W = ref_cols + 1;  // words of a diagonal
  uint64_t* diag = reinterpret_cast<uint64_t*>(smem);
  int32_t* s_h = reinterpret_cast<int32_t*>(diag + 3 * (int64_t)W);
  int32_t* s_r = s_h + hyp_cols;
  const int pair = blockIdx.x, rp = pair / R;
  const int tid = threadIdx.x, T = blockDim.x;

  int hl = hyp_len ? hyp_len[pair] : hyp_cols, rl = ref_len ? ref_len[rp] : ref_cols;
  hl = hl < 0 ? 0 : (hl > hyp_cols ? hyp_cols : hl);
  rl = rl < 0 ? 0 : (rl > ref_cols ? ref_cols : rl);
  const int n = ed_compact(hyp + (int64_t)pair * hyp_ld, hl, stop_id, skip_lo, skip_hi, s_h, s_w);
  const int m = ed_compact(ref + (int64_t)rp * ref_ld, rl, stop_id, skip_lo, skip_hi, s_r, s_w);
  int32_t* __restrict__ o = out + (int64_t)pair * out_ld;

  if (n == 0 || m == 0) {  // (uniform) C[n][0] = (n, 0, 0, n), C[0][m] = (m, 0, m, 0)
    if (tid == 0) o[0] = n + m, o[1] = 0, o[2] = m, o[3] = n, o[4] = n, o[5] = m;
    return;
  }
  for (int k = 0; k <= n + m; ++k) {  // (every thread runs every diagonal: the barrier is uniform)
    uint64_t* cur = diag + (k % 3) * W;
    const uint64_t* p1 = diag + ((k + 2) % 3) * W;  // diagonal k - 1
    const uint64_t* p2 = diag + ((k + 1) % 3) * W;  // diagonal k - 2
    const int jlo = k - n > 0 ? k - n : 0, jhi = k < m ? k : m;
    for (int j = jlo + tid; j <= jhi; j += T) {
      const int i = k - j;
      uint64_t c;
      if (i == 0) {
        c = (uint64_t)j | ((uint64_t)j << 28);
      } else if (j == 0) {
        c = (uint64_t)i | ((uint64_t)i << 42);
      } else {
        c = p2[j - 1] + (s_h[i - 1] != s_r[j - 1] ? ED_SUB : 0ull);
        const uint64_t up = p1[j] + ED_INS, lf = p1[j - 1] + ED_DEL;
        if ((up & ED_D) < (c & ED_D)) c = up;
        if ((lf & ED_D) < (c & ED_D)) c = lf;
      }
      cur[j] = c;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const uint64_t c = diag[((n + m) % 3) * W + m];
    o[0] = (int32_t)(c & ED_D), o[1] = (int32_t)((c >> 14) & ED_D), o[2] = (int32_t)((c >> 28) & ED_D);
    o[3] = (int32_t)((c >> 42) & ED_D), o[4] = n, o[5] = m;
  }
}

}  // namespace

static int tmi_edit_distance_impl(const int32_t* hyp, int64_t hyp_ld, int64_t hyp_cols, const int32_t* hyp_len,
                                  const int32_t* ref, int64_t ref_ld, int64_t ref_cols, const int32_t* ref_len, int64_t N,
                                  int64_t R, int32_t stop_id, int32_t skip_lo, int32_t skip_hi, int32_t* out, int64_t out_ld,
                                  void* stream) {
  const int64_t lim = (int64_t)1 << 30;
  if (!hyp || !ref || !out || !tmi_aligned(hyp, 4) || !tmi_aligned(ref, 4) || !tmi_aligned(out, 4) || !tmi_aligned(hyp_len, 4) ||
      !tmi_aligned(ref_len, 4) || N < 1 || N > 65535 || R < 1 || N % R != 0 || hyp_cols < 0 || hyp_cols > ED_MAXC || ref_cols < 0 ||
      ref_cols > ED_MAXC || hyp_ld < hyp_cols || hyp_ld > lim || ref_ld < ref_cols || ref_ld > lim || out_ld < 6 || out_ld > lim) {
    tmi_set_error("tmi_edit_distance: bad argument (hyp, ref, out non-NULL, every pointer 4-byte aligned; 1 <= N <= 65535, "
                  "R >= 1 dividing N; 0 <= hyp_cols, ref_cols <= 4096; hyp_ld >= hyp_cols, ref_ld >= ref_cols, out_ld >= 6)");
    return TMI_ERR_INVALID;
  }
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(edit_distance_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)ed_lds_bytes(ED_MAXC, ED_MAXC));
  (void)attr;
  int64_t threads = (ref_cols + TMI_WAVE - 1) / TMI_WAVE * TMI_WAVE;
  threads = threads < TMI_WAVE ? TMI_WAVE : (threads > ED_THREADS ? ED_THREADS : threads);
  hipLaunchKernelGGL(edit_distance_kernel, dim3((unsigned)N), dim3((unsigned)threads), (size_t)ed_lds_bytes(hyp_cols, ref_cols),
                     reinterpret_cast<hipStream_t>(stream), hyp, hyp_ld, (int)hyp_cols, hyp_len, ref, ref_ld, (int)ref_cols, ref_len,
                     (int)R, stop_id, skip_lo, skip_hi, out, out_ld);
  return tmi_check_launch("tmi_edit_distance");
}

extern "C" int tmi_edit_distance(const int32_t* hyp, int64_t hyp_ld, int64_t hyp_cols, const int32_t* hyp_len, const int32_t* ref,
                                 int64_t ref_ld, int64_t ref_cols, const int32_t* ref_len, int64_t N, int64_t R, int32_t stop_id,
                                 int32_t skip_lo, int32_t skip_hi, int32_t* out, int64_t out_ld, void* stream) {
  return tmi_plan_run<tmi_edit_distance_impl>(hyp, hyp_ld, hyp_cols, hyp_len, ref, ref_ld, ref_cols, ref_len, N, R, stop_id,
                                              skip_lo, skip_hi, out, out_ld, stream);
}
