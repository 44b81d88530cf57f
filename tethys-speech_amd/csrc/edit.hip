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
//
// tmi_edit_align is the same compaction and the same sweep (one template each, the flag off being tmi_edit_distance's
// code) plus:
//   Columns.  The compaction also keeps the source column of every kept token, 16 bits each, behind the tokens in LDS
//   (+ (hyp_cols + ref_cols) 2 bytes: 147480 at the limits, of the CU's 163840).
//   Moves.  A cell's move is 0 diagonal, 1 up, 2 left.  The lanes of a wave own 64 neighbouring cells of a diagonal, so
//   two ballots give the low and the high move bits of the 64 cells as two 64-bit words, which lane 0 stores as four
//   dwords: no read-modify-write of a packed word.  Workspace of pair p, as dwords:
//     ws[((p D + k) G + g) 4 + {0, 1}] = low bits, + {2, 3} = high bits of the cells j = jlo(k) + 64 g + b of diagonal k,
//     jlo(k) = max(0, k - n), D = hyp_cols + ref_cols + 1 diagonals, G = (min(hyp_cols, ref_cols) + 64) / 64 groups
//   (16 D G bytes a pair: 8.5 MB at the limits, 115 KB at 448 x 448).  Border cells are inside the words with bits that
//   nobody reads; every interior cell's word is written by the sweep, so the workspace's contents do not matter.
//   Trace.  After a block fence and a barrier thread 0 walks from (n, m) to (0, 0): at most n + m steps of two dependent
//   dword loads each (the words were just written by this workgroup).  n_steps = m + ins is known from the final cell,
//   so the steps are written from the back, already in forward order.
// tmi_edit_confusion: one workgroup of 256 threads per pair, a thread per step, one global integer atomic add per
// step (integer adds commute: the table does not depend on their order).
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
// the workgroup calls it; s_w is ED_WAVES words of LDS.  Ends on a barrier.  COLS: col[k] = the column of dst[k] in `row`.
template <bool COLS>
__device__ int ed_compact(const int32_t* __restrict__ row, int len, int32_t stop_id, int32_t skip_lo, int32_t skip_hi,
                          int32_t* dst, uint16_t* col, int* s_w) {
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
    if (keep) {
      const int at = off + __popcll(bal & ((1ull << lane) - 1ull));
      dst[at] = x;
      if constexpr (COLS) col[at] = (uint16_t)p;
    }
    __syncthreads();
  }
  return base;
}

// The table of n x m kept tokens, n, m >= 1, by anti-diagonals; ends on a barrier with C[n][m] at
// diag[((n + m) % 3) * W + m].  MOVES: the winning candidate of every cell goes to `mv` (this pair's words; the layout
// is at the top of the file), G groups a diagonal.
template <bool MOVES>
__device__ __forceinline__ void ed_sweep(uint64_t* diag, int W, const int32_t* s_h, const int32_t* s_r, int n, int m,
                                         uint32_t* mv, int G) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int k = 0; k <= n + m; ++k) {  // (every thread runs every diagonal: the barrier is uniform)
    uint64_t* cur = diag + (k % 3) * W;
    const uint64_t* p1 = diag + ((k + 2) % 3) * W;  // diagonal k - 1
    const uint64_t* p2 = diag + ((k + 1) % 3) * W;  // diagonal k - 2
    const int jlo = k - n > 0 ? k - n : 0, jhi = k < m ? k : m;
    for (int j = jlo + tid; j <= jhi; j += T) {
      const int i = k - j;
      uint64_t c;
      int move = 0;
      if (i == 0) {
        c = (uint64_t)j | ((uint64_t)j << 28);
      } else if (j == 0) {
        c = (uint64_t)i | ((uint64_t)i << 42);
      } else {
        c = p2[j - 1] + (s_h[i - 1] != s_r[j - 1] ? ED_SUB : 0ull);
        const uint64_t up = p1[j] + ED_INS, lf = p1[j - 1] + ED_DEL;
        if ((up & ED_D) < (c & ED_D)) c = up, move = 1;
        if ((lf & ED_D) < (c & ED_D)) c = lf, move = 2;
      }
      cur[j] = c;
      if constexpr (MOVES) {  // the lanes in the loop are a prefix of the wave: lane 0 is among them
        const unsigned long long lo = __ballot(move & 1), hi = __ballot(move >> 1);
        if ((tid & 63) == 0) {
          uint32_t* w = mv + ((int64_t)k * G + ((j - jlo) >> 6)) * 4;
          w[0] = (uint32_t)lo, w[1] = (uint32_t)(lo >> 32), w[2] = (uint32_t)hi, w[3] = (uint32_t)(hi >> 32);
        }
      }
    }
    __syncthreads();
  }
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
  const int n = ed_compact<false>(hyp + (int64_t)pair * hyp_ld, hl, stop_id, skip_lo, skip_hi, s_h, nullptr, s_w);
  const int m = ed_compact<false>(ref + (int64_t)rp * ref_ld, rl, stop_id, skip_lo, skip_hi, s_r, nullptr, s_w);
  int32_t* __restrict__ o = out + (int64_t)pair * out_ld;

  if (n == 0 || m == 0) {  // (uniform) C[n][0] = (n, 0, 0, n), C[0][m] = (m, 0, m, 0)
    if (tid == 0) o[0] = n + m, o[1] = 0, o[2] = m, o[3] = n, o[4] = n, o[5] = m;
    return;
  }
  ed_sweep<false>(diag, W, s_h, s_r, n, m, nullptr, 0);
  if (tid == 0) {
    const uint64_t c = diag[((n + m) % 3) * W + m];
    o[0] = (int32_t)(c & ED_D), o[1] = (int32_t)((c >> 14) & ED_D), o[2] = (int32_t)((c >> 28) & ED_D);
    o[3] = (int32_t)((c >> 42) & ED_D), o[4] = n, o[5] = m;
  }
}

constexpr int64_t ea_lds_bytes(int64_t hyp_cols, int64_t ref_cols) { return ed_lds_bytes(hyp_cols, ref_cols) + (hyp_cols + ref_cols) * 2; }
constexpr int64_t ea_groups(int64_t hyp_cols, int64_t ref_cols) { return ((hyp_cols < ref_cols ? hyp_cols : ref_cols) + 64) / 64; }

__global__ __launch_bounds__(ED_THREADS) void edit_align_kernel(
    const int32_t* __restrict__ hyp, int64_t hyp_ld, int hyp_cols, const int32_t* __restrict__ hyp_len,
    const int32_t* __restrict__ ref, int64_t ref_ld, int ref_cols, const int32_t* __restrict__ ref_len, int R,
    int32_t stop_id, int32_t skip_lo, int32_t skip_hi, int32_t* __restrict__ out, int64_t out_ld, int32_t* __restrict__ steps,
    int64_t steps_ld, int32_t* __restrict__ n_steps, uint32_t* ws) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ int s_w[ED_WAVES];
  const int W = ref_cols + 1;  // words of a diagonal
  uint64_t* diag = reinterpret_cast<uint64_t*>(smem);
  int32_t* s_h = reinterpret_cast<int32_t*>(diag + 3 * (int64_t)W);
  int32_t* s_r = s_h + hyp_cols;
  uint16_t* c_h = reinterpret_cast<uint16_t*>(s_r + ref_cols);  // the columns of the kept tokens
  uint16_t* c_r = c_h + hyp_cols;
  const int pair = blockIdx.x, rp = pair / R;
  const int tid = threadIdx.x, T = blockDim.x;

  int hl = hyp_len ? hyp_len[pair] : hyp_cols, rl = ref_len ? ref_len[rp] : ref_cols;
  hl = hl < 0 ? 0 : (hl > hyp_cols ? hyp_cols : hl);
  rl = rl < 0 ? 0 : (rl > ref_cols ? ref_cols : rl);
  const int n = ed_compact<true>(hyp + (int64_t)pair * hyp_ld, hl, stop_id, skip_lo, skip_hi, s_h, c_h, s_w);
  const int m = ed_compact<true>(ref + (int64_t)rp * ref_ld, rl, stop_id, skip_lo, skip_hi, s_r, c_r, s_w);
  int32_t* __restrict__ o = out + (int64_t)pair * out_ld;
  int32_t* __restrict__ st = steps + (int64_t)pair * steps_ld;

  if (n == 0 || m == 0) {  // (uniform) m deletions, n insertions or nothing
    for (int k = tid; k < n + m; k += T) {
      st[3 * k] = n ? 3 : 2;
      st[3 * k + 1] = n ? (int32_t)c_h[k] : -1;
      st[3 * k + 2] = n ? -1 : (int32_t)c_r[k];
    }
    if (tid == 0) o[0] = n + m, o[1] = 0, o[2] = m, o[3] = n, o[4] = n, o[5] = m, n_steps[pair] = n + m;
    return;
  }
  const int G = (int)ea_groups(hyp_cols, ref_cols);
  uint32_t* mv = ws + (int64_t)pair * (hyp_cols + ref_cols + 1) * G * 4;
  ed_sweep<true>(diag, W, s_h, s_r, n, m, mv, G);
  __threadfence_block();  // the move words of every wave, before thread 0 reads them
  __syncthreads();
  if (tid == 0) {
    const uint64_t c = diag[((n + m) % 3) * W + m];
    const int ins = (int)((c >> 42) & ED_D), total = m + ins;  // == n + del
    o[0] = (int32_t)(c & ED_D), o[1] = (int32_t)((c >> 14) & ED_D), o[2] = (int32_t)((c >> 28) & ED_D);
    o[3] = ins, o[4] = n, o[5] = m, n_steps[pair] = total;
#ifndef TMI_EDIT_ALIGN_NO_TRACE  // (tools/edit_align_bench.py builds a private copy without the walk, to time the sweep alone)
    int i = n, j = m;
    for (int k = total - 1; k >= 0 && (i > 0 || j > 0); --k) {
      int move;
      if (i == 0) {
        move = 2;
      } else if (j == 0) {
        move = 1;
      } else {
        const int dg = i + j, p = j - (dg - n > 0 ? dg - n : 0);
        const uint32_t* w = mv + ((int64_t)dg * G + (p >> 6)) * 4 + ((p >> 5) & 1);
        move = (int)((w[0] >> (p & 31)) & 1u) | ((int)((w[2] >> (p & 31)) & 1u) << 1);
      }
      if (move == 0) {
        st[3 * k] = s_h[i - 1] != s_r[j - 1], st[3 * k + 1] = c_h[i - 1], st[3 * k + 2] = c_r[j - 1];
        --i, --j;
      } else if (move == 1) {
        st[3 * k] = 3, st[3 * k + 1] = c_h[i - 1], st[3 * k + 2] = -1;
        --i;
      } else {
        st[3 * k] = 2, st[3 * k + 1] = -1, st[3 * k + 2] = c_r[j - 1];
        --j;
      }
    }
#endif
  }
}

constexpr int EC_THREADS = 256;

__global__ __launch_bounds__(EC_THREADS) void edit_confusion_kernel(
    const int32_t* __restrict__ steps, int64_t steps_ld, const int32_t* __restrict__ n_steps, const int32_t* __restrict__ hyp,
    int64_t hyp_ld, int hyp_cols, const int32_t* __restrict__ ref, int64_t ref_ld, int ref_cols, int R, int first_only, int V,
    int32_t* counts) {
  const int pair = blockIdx.x, rp = pair / R;
  if (first_only && pair % R != 0) return;
  int ns = n_steps[pair];
  ns = ns < 0 ? 0 : (ns > hyp_cols + ref_cols ? hyp_cols + ref_cols : ns);
  const int32_t* st = steps + (int64_t)pair * steps_ld;
  const int32_t* h = hyp + (int64_t)pair * hyp_ld;
  const int32_t* r = ref + (int64_t)rp * ref_ld;
  for (int k = threadIdx.x; k < ns; k += EC_THREADS) {
    const int op = st[3 * k], ch = st[3 * k + 1], cr = st[3 * k + 2];
    // row = the reference token, column = the hypothesis token, V = none; anything that cannot be indexed stays -1
    int row = -1, col = -1;
    if (op == 3) row = V;
    else if (op >= 0 && op < 3 && cr >= 0 && cr < ref_cols) row = r[cr];
    if (op == 2) col = V;
    else if (op >= 0 && op <= 3 && ch >= 0 && ch < hyp_cols) col = h[ch];
    const bool ok = row >= 0 && row <= V && col >= 0 && col <= V && (op == 3 || row < V) && (op == 2 || col < V);
    atomicAdd(counts + (ok ? (int64_t)row * (V + 1) + col : (int64_t)(V + 1) * (V + 1)), 1);
  }
}

}  // namespace

static bool ed_rows_ok(const int32_t* hyp, int64_t hyp_ld, int64_t hyp_cols, const int32_t* ref, int64_t ref_ld, int64_t ref_cols,
                       int64_t N, int64_t R) {
  const int64_t lim = (int64_t)1 << 30;
  return hyp && ref && tmi_aligned(hyp, 4) && tmi_aligned(ref, 4) && N >= 1 && N <= 65535 && R >= 1 && N % R == 0 && hyp_cols >= 0 &&
         hyp_cols <= ED_MAXC && ref_cols >= 0 && ref_cols <= ED_MAXC && hyp_ld >= hyp_cols && hyp_ld <= lim && ref_ld >= ref_cols &&
         ref_ld <= lim;
}

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

extern "C" int64_t tmi_edit_align_workspace_bytes(int64_t N, int64_t hyp_cols, int64_t ref_cols) {
  if (N < 1 || N > 65535 || hyp_cols < 0 || hyp_cols > ED_MAXC || ref_cols < 0 || ref_cols > ED_MAXC) return -1;
  return N * (hyp_cols + ref_cols + 1) * ea_groups(hyp_cols, ref_cols) * 16;
}

static int tmi_edit_align_impl(const int32_t* hyp, int64_t hyp_ld, int64_t hyp_cols, const int32_t* hyp_len, const int32_t* ref,
                               int64_t ref_ld, int64_t ref_cols, const int32_t* ref_len, int64_t N, int64_t R, int32_t stop_id,
                               int32_t skip_lo, int32_t skip_hi, int32_t* out, int64_t out_ld, int32_t* steps, int64_t steps_ld,
                               int32_t* n_steps, void* workspace, int64_t workspace_bytes, void* stream) {
  const int64_t lim = (int64_t)1 << 30;
  if (!ed_rows_ok(hyp, hyp_ld, hyp_cols, ref, ref_ld, ref_cols, N, R) || !out || !steps || !n_steps || !workspace ||
      !tmi_aligned(out, 4) || !tmi_aligned(hyp_len, 4) || !tmi_aligned(ref_len, 4) || !tmi_aligned(steps, 4) ||
      !tmi_aligned(n_steps, 4) || !tmi_aligned(workspace, 4) || out_ld < 6 || out_ld > lim || steps_ld < 3 * (hyp_cols + ref_cols) ||
      steps_ld > lim || workspace_bytes < tmi_edit_align_workspace_bytes(N, hyp_cols, ref_cols)) {
    tmi_set_error("tmi_edit_align: bad argument (tmi_edit_distance's conditions; steps, n_steps, workspace non-NULL and 4-byte "
                  "aligned; steps_ld >= 3 (hyp_cols + ref_cols); workspace of tmi_edit_align_workspace_bytes)");
    return TMI_ERR_INVALID;
  }
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(edit_align_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)ea_lds_bytes(ED_MAXC, ED_MAXC));
  (void)attr;
  int64_t threads = (ref_cols + TMI_WAVE - 1) / TMI_WAVE * TMI_WAVE;
  threads = threads < TMI_WAVE ? TMI_WAVE : (threads > ED_THREADS ? ED_THREADS : threads);
  hipLaunchKernelGGL(edit_align_kernel, dim3((unsigned)N), dim3((unsigned)threads), (size_t)ea_lds_bytes(hyp_cols, ref_cols),
                     reinterpret_cast<hipStream_t>(stream), hyp, hyp_ld, (int)hyp_cols, hyp_len, ref, ref_ld, (int)ref_cols, ref_len,
                     (int)R, stop_id, skip_lo, skip_hi, out, out_ld, steps, steps_ld, n_steps, reinterpret_cast<uint32_t*>(workspace));
  return tmi_check_launch("tmi_edit_align");
}

extern "C" int tmi_edit_align(const int32_t* hyp, int64_t hyp_ld, int64_t hyp_cols, const int32_t* hyp_len, const int32_t* ref,
                              int64_t ref_ld, int64_t ref_cols, const int32_t* ref_len, int64_t N, int64_t R, int32_t stop_id,
                              int32_t skip_lo, int32_t skip_hi, int32_t* out, int64_t out_ld, int32_t* steps, int64_t steps_ld,
                              int32_t* n_steps, void* workspace, int64_t workspace_bytes, void* stream) {
  return tmi_plan_run<tmi_edit_align_impl>(hyp, hyp_ld, hyp_cols, hyp_len, ref, ref_ld, ref_cols, ref_len, N, R, stop_id, skip_lo,
                                           skip_hi, out, out_ld, steps, steps_ld, n_steps, workspace, workspace_bytes, stream);
}

static int tmi_edit_confusion_impl(const int32_t* steps, int64_t steps_ld, const int32_t* n_steps, const int32_t* hyp, int64_t hyp_ld,
                                   int64_t hyp_cols, const int32_t* ref, int64_t ref_ld, int64_t ref_cols, int64_t N, int64_t R,
                                   int32_t first_only, int64_t V, int32_t* counts, int32_t accumulate, void* stream) {
  if (!ed_rows_ok(hyp, hyp_ld, hyp_cols, ref, ref_ld, ref_cols, N, R) || !steps || !n_steps || !counts || !tmi_aligned(steps, 4) ||
      !tmi_aligned(n_steps, 4) || !tmi_aligned(counts, 4) || steps_ld < 3 * (hyp_cols + ref_cols) || steps_ld > ((int64_t)1 << 30) ||
      V < 1 || V > 1024 || (first_only != 0 && first_only != 1) || (accumulate != 0 && accumulate != 1)) {
    tmi_set_error("tmi_edit_confusion: bad argument (the rows and strides of tmi_edit_align's call; steps, n_steps, counts non-NULL "
                  "and 4-byte aligned; 1 <= V <= 1024; first_only, accumulate 0 or 1)");
    return TMI_ERR_INVALID;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!accumulate && hipMemsetAsync(counts, 0, (size_t)((V + 1) * (V + 1) + 1) * 4, s) != hipSuccess) {
    tmi_set_error("tmi_edit_confusion: the counts could not be zeroed");
    return TMI_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(edit_confusion_kernel, dim3((unsigned)N), dim3(EC_THREADS), 0, s, steps, steps_ld, n_steps, hyp, hyp_ld,
                     (int)hyp_cols, ref, ref_ld, (int)ref_cols, (int)R, (int)first_only, (int)V, counts);
  return tmi_check_launch("tmi_edit_confusion");
}

extern "C" int tmi_edit_confusion(const int32_t* steps, int64_t steps_ld, const int32_t* n_steps, const int32_t* hyp, int64_t hyp_ld,
                                  int64_t hyp_cols, const int32_t* ref, int64_t ref_ld, int64_t ref_cols, int64_t N, int64_t R,
                                  int32_t first_only, int64_t V, int32_t* counts, int32_t accumulate, void* stream) {
  return tmi_plan_run<tmi_edit_confusion_impl>(steps, steps_ld, n_steps, hyp, hyp_ld, hyp_cols, ref, ref_ld, ref_cols, N, R, first_only,
                                               V, counts, accumulate, stream);
}
