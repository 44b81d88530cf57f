// SpecAugment span masks for the probes on cached features (apply_time_mask / apply_feature_mask, V:1073-1119):
// tmi_spec_masks draws the masks as bits, tmi_span_mask_apply zeroes a tensor under them.  include/tethys_mi.h states the
// contract; this is how it is carried out.  Integers only: the same call gives the same bits.
//
// spec_masks_kernel - one workgroup of 256 threads per (item n, mask m): m = 0 the time mask over T_max frames (stream 1),
//   m = 1 the feature mask over H columns (stream 2).  A wave owns 64 consecutive columns at a time (chunk k: the columns
//   64 k .. 64 k + 63; wave w the chunks w, w + 4, ..).  Lane l draws the start of its own column c = 64 k + l and of the
//   column c - 64 (two evaluations of tmi_keep), and two ballots give the 128 start bits of the columns 64 k - 64 ..
//   64 k + 63.  mask = OR of the starts shifted up by 0 .. length - 1: the window is widened by doubling (1, 2, 4, ..; the
//   last shift is what is left of `length`), at most 6 shift-ORs of the 128 bits, and because length <= 64 no start before
//   64 k - 64 can reach the chunk.  The upper 64 bits, cut at `cols`, are the chunk's mask: lane 0 writes its one or two
//   words.  The wave adds the chunks' popcounts; thread 0 adds the four waves' sums: counts[n][m].
// span_mask_apply_kernel - one thread per 8 consecutive columns of one frame, moved as raw bits (16-byte accesses when
//   the strides and pointers allow it, element accesses otherwise): a masked element becomes +0, the others are copied.
#include "tmi_common.h"

namespace {

constexpr int SA_THREADS = 256;
constexpr int64_t SA_MAXN = 65535, SA_MAXT = 4096, SA_MAXROWS = (int64_t)1 << 22, SA_MAXH = 4096, SA_MAXLEN = 64;
constexpr uint32_t SA_STREAM_TIME = 1, SA_STREAM_FEAT = 2;

struct span_t {  // one of the two masks
  uint32_t* bits;
  int64_t ld;
  uint32_t key, thr;
  int cols, length;
};

__global__ __launch_bounds__(SA_THREADS) void spec_masks_kernel(span_t tm, span_t fm, int32_t* __restrict__ counts) {
  __shared__ int red[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = blockIdx.x;
  const span_t s = blockIdx.y == 0 ? tm : fm;
  int cnt = 0;
  if (s.bits != nullptr) {
    uint32_t* __restrict__ row = s.bits + (int64_t)n * s.ld;
    const int nwords = (s.cols + 31) >> 5;
    for (int k = wv; k * 64 < s.cols; k += 4) {  // (uniform over the wave)
      const int c = k * 64 + lane;
      bool s_own = false, s_prev = false;
      if (s.thr != 0) {  // prob == 0: nothing is hashed
        s_own = c < s.cols && !tmi_keep(s.key, (uint32_t)n, (uint32_t)c, s.thr);
        s_prev = c >= 64 && !tmi_keep(s.key, (uint32_t)n, (uint32_t)(c - 64), s.thr);
      }
      uint64_t hi = __ballot(s_own), lo = __ballot(s_prev);
      for (int done = 1; done < s.length;) {  // the window covers `done` columns; sh <= 32
        const int sh = s.length - done < done ? s.length - done : done;
        hi = (hi << sh) | (hi | (lo >> (64 - sh)));
        lo |= lo << sh;
        done += sh;
      }
      const int left = s.cols - k * 64;
      if (left < 64) hi &= ((uint64_t)1 << left) - 1;
      cnt += __popcll(hi);
      if (lane == 0) {
        row[2 * k] = (uint32_t)hi;
        if (2 * k + 1 < nwords) row[2 * k + 1] = (uint32_t)(hi >> 32);
      }
    }
  }
  if (counts == nullptr) return;
  if (lane == 0) red[wv] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) counts[2 * n + blockIdx.y] = (red[0] + red[1]) + (red[2] + red[3]);
}

template <typename U>
__global__ __launch_bounds__(SA_THREADS) void span_mask_apply_kernel(const U* __restrict__ x, int64_t x_sn, int64_t x_st,
                                                                    const uint32_t* __restrict__ time_bits, int64_t ld_t,
                                                                    const uint32_t* __restrict__ feat_bits, int64_t ld_f,
                                                                    U* __restrict__ out, int64_t o_sn, int64_t o_st, int64_t rows,
                                                                    int T, int H, bool vec) {
  constexpr int NV = (int)sizeof(U) * 8 / 16;  // 16-byte pieces of 8 elements
  const int H8 = H >> 3;
  const int64_t e = (int64_t)blockIdx.x * SA_THREADS + threadIdx.x;
  const int64_t r = e / H8;
  if (r >= rows) return;
  const int c = (int)(e - r * H8) * 8;
  const int n = (int)(r / T), t = (int)(r - (int64_t)n * T);
  uint32_t m = 0;  // bit i: column c + i is masked
  if (time_bits != nullptr && ((time_bits[(int64_t)n * ld_t + (t >> 5)] >> (t & 31)) & 1u)) m = 0xffu;
  if (feat_bits != nullptr) m |= (feat_bits[(int64_t)n * ld_f + (c >> 5)] >> (c & 31)) & 0xffu;
  const U* __restrict__ p = x + (int64_t)n * x_sn + (int64_t)t * x_st + c;
  U* __restrict__ o = out + (int64_t)n * o_sn + (int64_t)t * o_st + c;
  union {
    U v[8];
    u32x4 q[NV];
  } u;
  if (vec) {
#pragma unroll
    for (int i = 0; i < NV; ++i) u.q[i] = reinterpret_cast<const u32x4*>(p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) u.v[i] = p[i];
  }
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if ((m >> i) & 1u) u.v[i] = 0;
  if (vec) {
#pragma unroll
    for (int i = 0; i < NV; ++i) reinterpret_cast<u32x4*>(o)[i] = u.q[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = u.v[i];
  }
}

bool sa_sizes_ok(int64_t N, int64_t T_max, int64_t H) {
  return N >= 1 && N <= SA_MAXN && T_max >= 1 && T_max <= SA_MAXT && N * T_max <= SA_MAXROWS && H >= 8 && H <= SA_MAXH &&
         H % 8 == 0;
}
bool sa_span_ok(float prob, int64_t length) {
  return prob >= 0.f && prob < 1.f && tmi_drop_ok(prob) && length >= 1 && length <= SA_MAXLEN;
}
// (NULL: that mask is off and its ld is not looked at)
bool sa_bits_ok(const uint32_t* bits, int64_t ld, int64_t cols) {
  return bits == nullptr || (tmi_aligned(bits, 4) && ld >= (cols + 31) / 32 && ld <= ((int64_t)1 << 30));
}
bool sa_stride_ok(int64_t sn, int64_t st, int64_t T, int64_t H) {
  const int64_t lim = (int64_t)1 << 30;
  return st >= H && st <= lim && sn >= T * st && sn <= lim;
}

}  // namespace

static int tmi_spec_masks_impl(uint32_t* time_bits, int64_t ld_t, uint32_t* feat_bits, int64_t ld_f, int32_t* counts, int64_t N,
                               int64_t T_max, int64_t H, float time_prob, int64_t time_length, float feat_prob,
                               int64_t feat_length, uint64_t seed, void* stream) {
  const bool ok = sa_sizes_ok(N, T_max, H) && (time_bits != nullptr || feat_bits != nullptr) &&
                  (time_bits == nullptr || sa_span_ok(time_prob, time_length)) &&
                  (feat_bits == nullptr || sa_span_ok(feat_prob, feat_length)) && sa_bits_ok(time_bits, ld_t, T_max) &&
                  sa_bits_ok(feat_bits, ld_f, H) && tmi_aligned(counts, 4);
  if (!ok) {
    tmi_set_error("tmi_spec_masks: bad argument (1 <= N <= 65535; 1 <= T_max <= 4096; N*T_max <= 2^22; 8 <= H <= 4096, a multiple "
                  "of 8; time_bits or feat_bits non-NULL; for a mask that is not NULL: 0 <= prob < 1, 1 <= length <= 64, ld >= "
                  "ceil(columns / 32) and <= 2^30; pointers 4-byte aligned)");
    return TMI_ERR_INVALID;
  }
  span_t tm, fm;
  tm.bits = time_bits, tm.ld = ld_t, tm.cols = (int)T_max, tm.length = (int)time_length;
  tm.key = tmi_stream_key(seed, SA_STREAM_TIME), tm.thr = time_bits ? tmi_drop_thr(time_prob) : 0;
  fm.bits = feat_bits, fm.ld = ld_f, fm.cols = (int)H, fm.length = (int)feat_length;
  fm.key = tmi_stream_key(seed, SA_STREAM_FEAT), fm.thr = feat_bits ? tmi_drop_thr(feat_prob) : 0;
  hipLaunchKernelGGL(spec_masks_kernel, dim3((unsigned)N, 2), dim3(SA_THREADS), 0, reinterpret_cast<hipStream_t>(stream), tm, fm,
                     counts);
  return tmi_check_launch("tmi_spec_masks");
}

extern "C" int tmi_spec_masks(uint32_t* time_bits, int64_t ld_t, uint32_t* feat_bits, int64_t ld_f, int32_t* counts, int64_t N,
                              int64_t T_max, int64_t H, float time_prob, int64_t time_length, float feat_prob, int64_t feat_length,
                              uint64_t seed, void* stream) {
  return tmi_plan_run<tmi_spec_masks_impl>(time_bits, ld_t, feat_bits, ld_f, counts, N, T_max, H, time_prob, time_length, feat_prob,
                                           feat_length, tmi_plan_seed{seed}, stream);
}

static int tmi_span_mask_apply_impl(const void* x, int32_t x_dtype, int64_t x_sn, int64_t x_st, const uint32_t* time_bits,
                                    int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* out, int64_t o_sn, int64_t o_st,
                                    int64_t N, int64_t T, int64_t H, void* stream) {
  const int64_t es = x_dtype == TMI_BF16 ? 2 : 4;
  const bool ok = sa_sizes_ok(N, T, H) && (x_dtype == TMI_F32 || x_dtype == TMI_BF16) && x != nullptr && out != nullptr &&
                  tmi_aligned(x, es) && tmi_aligned(out, es) && sa_stride_ok(x_sn, x_st, T, H) && sa_stride_ok(o_sn, o_st, T, H) &&
                  sa_bits_ok(time_bits, ld_t, T) && sa_bits_ok(feat_bits, ld_f, H);
  if (!ok) {
    tmi_set_error("tmi_span_mask_apply: bad argument (1 <= N <= 65535; 1 <= T <= 4096; N*T <= 2^22; 8 <= H <= 4096, a multiple of "
                  "8; x_dtype TMI_F32 or TMI_BF16; x and out non-NULL and aligned to an element; x_st, o_st >= H, item strides >= "
                  "T * the frame stride, all <= 2^30; a mask NULL or 4-byte aligned with ld >= ceil(columns / 32))");
    return TMI_ERR_INVALID;
  }
  const int64_t q = 16 / es;  // elements per 16 bytes
  const bool vec = x_sn % q == 0 && x_st % q == 0 && o_sn % q == 0 && o_st % q == 0 && tmi_aligned(x, 16) && tmi_aligned(out, 16);
  const int64_t threads = N * T * (H / 8);
  const dim3 grid((unsigned)((threads + SA_THREADS - 1) / SA_THREADS));
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (x_dtype == TMI_BF16)
    hipLaunchKernelGGL(span_mask_apply_kernel<uint16_t>, grid, dim3(SA_THREADS), 0, st, reinterpret_cast<const uint16_t*>(x), x_sn,
                       x_st, time_bits, ld_t, feat_bits, ld_f, reinterpret_cast<uint16_t*>(out), o_sn, o_st, N * T, (int)T, (int)H,
                       vec);
  else
    hipLaunchKernelGGL(span_mask_apply_kernel<uint32_t>, grid, dim3(SA_THREADS), 0, st, reinterpret_cast<const uint32_t*>(x), x_sn,
                       x_st, time_bits, ld_t, feat_bits, ld_f, reinterpret_cast<uint32_t*>(out), o_sn, o_st, N * T, (int)T, (int)H,
                       vec);
  return tmi_check_launch("tmi_span_mask_apply");
}

extern "C" int tmi_span_mask_apply(const void* x, int32_t x_dtype, int64_t x_sn, int64_t x_st, const uint32_t* time_bits,
                                   int64_t ld_t, const uint32_t* feat_bits, int64_t ld_f, void* out, int64_t o_sn, int64_t o_st,
                                   int64_t N, int64_t T, int64_t H, void* stream) {
  return tmi_plan_run<tmi_span_mask_apply_impl>(x, x_dtype, x_sn, x_st, time_bits, ld_t, feat_bits, ld_f, out, o_sn, o_st, N, T, H,
                                                stream);
}
