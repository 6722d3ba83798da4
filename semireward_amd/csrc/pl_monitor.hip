// Pseudo-label quality monitor (``monitor_pseudo_labels: True``, semireward_amd/core/pl_monitor.py): ONE launch per training step that adds what
// the step's masks, pseudo labels, rewards and reward filter say about the TRUE labels of the unlabelled rows into device-resident counters.
// The host reads the counters once per log line; nothing here is on the step's dependency chain.  include/srhip.h holds the contract
// (semantics, state layout).
//
// A launch covers at most a few thousand elements (9 x 56 at the reference batch, 9 x 448 at Bu = 64): ONE workgroup of 4 waves, so that the
// whole reduction stays in the launch without a scratch buffer -- the launch latency is the cost, not the work (9 x 448: two row items and
// four quad items per thread).
//   * two item kinds share the thread index space: ROW items (row j: bounds, pass 0, the kept pass) and QUAD items (four consecutive elements
//     of the flat [K * nu] reward / mask2 arrays and of pseudo + nu: the data_generator passes).  A quad is an aligned 16-byte load of
//     reward and of mask2 when both bases allow; the quad holding the end is peeled.  Items are strided over the threads in a fixed order, the
//     same in the 16-byte and the scalar instantiation: both give the same bits.
//   * the true label of every row (idx_ulb -> ulb_targets, a dependent gather) is staged in LDS once, for the rows j < 2048; rows beyond
//     that are gathered at every use.
//   * integer counters: per thread in registers, a wave butterfly, one LDS add per wave and counter; the histogram and (C <= 2048) the
//     per-class counters are LDS integer atomics, flushed by plain read-modify-writes (one workgroup, launches of a stream are ordered);
//     C > 2048: the per-class counters are global 64-bit integer atomics.  Integer sums do not depend on the order.
//   * fp64 sums: per-thread partials in item order, a wave butterfly, one thread per sum adds the 4 wave sums in wave order -- no float atomics, a launch
//     is bitwise repeatable.
#include "common.h"
#include "srhip.h"

// op by op: w = mask * mask2 is ONE fp32 rounding, as the criterion kernels take it
#pragma clang fp contract(off)

namespace {

constexpr int WAVES = 4;
constexpr int THREADS = WAVES * 64;
constexpr int LDS_CLASSES = 2048;         // per-class counters in LDS up to this C (2 x 2048 x 4 B = 16 KB)
constexpr int LDS_ROWS = 2048;            // true labels of the rows j < 2048 staged in LDS (8 KB): one idx_ulb -> label gather per row, not K + 1
constexpr int HDR = 16;                   // int64 header words (srhip.h)
constexpr int NCNT = 12;                  // header counters a launch accumulates (words 1 .. 12; word 0 = steps)
constexpr int BINS = 32;
constexpr int ERR_BIT = 32;               // bit 5 of the label-error word

enum { ROWS = 0, ROWS_CORRECT, SEL, SEL_CORRECT, CONF_SEL, CONF_SEL_CORRECT, ROWS_UNKNOWN, GEN_ROWS, GEN_CORRECT, REWARD_BAD, M2, M2_CORRECT };
enum { SUM_W = 0, SUM_W_CORRECT, SUM_R_WRONG, SUM_R_RIGHT, NSUM };

struct MonArgs {
  const long long* pseudo;
  const float* mask0;
  const float* mask_kept;
  const float* mask2;
  const float* reward;
  const long long* idx_ulb;
  const long long* targets;
  long long* ist;
  double* fst;
  int* label_err;
  long long n_ulb;
  int K, nu, C;
};

// true label of weak row j: >= 0 known (< C <= 2^28: an int), -1 unknown, -2 out of bounds (nothing is read out of bounds)
__device__ __forceinline__ int true_label(const MonArgs& a, int j) {
  const long long i = a.idx_ulb[j];
  if (i < 0 || i >= a.n_ulb) return -2;
  const long long y = a.targets[i];
  if (y >= (long long)a.C) return -2;
  return y < 0 ? -1 : (int)y;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool VEC, bool LDS_CLS> __global__ __launch_bounds__(THREADS) void pl_monitor_kernel(MonArgs a) {
  __shared__ int cnt_s[NCNT];
  __shared__ int hist_s[2 * BINS];
  __shared__ int cls_s[LDS_CLS ? 2 * LDS_CLASSES : 1];
  __shared__ double part_s[WAVES][NSUM];
  __shared__ int y_s[LDS_ROWS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int K = a.K, nu = a.nu, C = a.C;
  if (tid < NCNT) cnt_s[tid] = 0;
  if (tid < 2 * BINS) hist_s[tid] = 0;
  if (LDS_CLS)
    for (int c = tid; c < 2 * C; c += THREADS) cls_s[c] = 0;
  for (int j = tid; j < min(nu, LDS_ROWS); j += THREADS) y_s[j] = true_label(a, j);
  __syncthreads();
  auto label = [&](int j) -> int { return j < LDS_ROWS ? y_s[j] : true_label(a, j); };      // rows beyond the staged ones: gathered each time

  int cnt[NCNT];
  double sum[NSUM];
#pragma unroll
  for (int i = 0; i < NCNT; ++i) cnt[i] = 0;
#pragma unroll
  for (int i = 0; i < NSUM; ++i) sum[i] = 0.0;
  long long* cls_g = a.ist + HDR;

  // ---- row items: bounds, pass 0 (the confidence mask alone), the kept pass f = K
  for (int j = tid; j < nu; j += THREADS) {
    const long long y = label(j);
    if (y == -2) { atomicOr(a.label_err, ERR_BIT); continue; }
    if (y < 0) { ++cnt[ROWS_UNKNOWN]; continue; }
    const float m0 = a.mask0[j];
    if (m0 > 0.f) {
      ++cnt[CONF_SEL];
      cnt[CONF_SEL_CORRECT] += a.pseudo[j] == y;
    }
    const long long pl = a.pseudo[(size_t)K * nu + j];
    const float w = K == 0 ? a.mask_kept[j] : a.mask_kept[j] * a.mask2[(size_t)(K - 1) * nu + j];
    const bool ok = pl == y, s = w > 0.f;
    ++cnt[ROWS];
    cnt[ROWS_CORRECT] += ok;
    cnt[SEL] += s;
    cnt[SEL_CORRECT] += s && ok;
    sum[SUM_W] += (double)w;
    if (ok) sum[SUM_W_CORRECT] += (double)w;
    if (s && pl >= 0 && pl < (long long)C) {
      if (LDS_CLS) {
        atomicAdd(&cls_s[(int)pl], 1);
        if (ok) atomicAdd(&cls_s[C + (int)pl], 1);
      } else {
        atomicAdd((unsigned long long*)(cls_g + pl), 1ull);
        if (ok) atomicAdd((unsigned long long*)(cls_g + C + pl), 1ull);
      }
    }
  }

  // ---- quad items: the data_generator passes g = 0 .. K - 1, flat element e = g * nu + j
  const long long n = (long long)K * nu;
  const long long* pg = a.pseudo + nu;
  for (long long e0 = 4ll * tid; e0 < n; e0 += 4ll * THREADS) {
    f32x4_t r4 = {0.f, 0.f, 0.f, 0.f}, q4 = {0.f, 0.f, 0.f, 0.f};
    if (VEC && e0 + 4 <= n) {
      r4 = *reinterpret_cast<const f32x4_t*>(a.reward + e0);
      q4 = *reinterpret_cast<const f32x4_t*>(a.mask2 + e0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (e0 + i < n) { r4[i] = a.reward[e0 + i]; q4[i] = a.mask2[e0 + i]; }
    }
    int j = (int)(e0 % nu);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (e0 + i < n) {
        const long long y = label(j);
        if (y >= 0) {
          const bool ok = pg[e0 + i] == y;
          const float r = r4[i];
          ++cnt[GEN_ROWS];
          cnt[GEN_CORRECT] += ok;
          if (q4[i] > 0.f) {
            ++cnt[M2];
            cnt[M2_CORRECT] += ok;
          }
          if (r >= 0.f && r <= 1.f) {
            const int b = min((int)(r * 32.0f), BINS - 1);
            atomicAdd(&hist_s[(ok ? BINS : 0) + b], 1);
            sum[ok ? SUM_R_RIGHT : SUM_R_WRONG] += (double)r;
          } else {
            ++cnt[REWARD_BAD];                                     // NaN or outside [0, 1]: not binned, not summed
          }
        }
      }
      if (++j == nu) j = 0;
    }
  }

  // ---- reductions: integers in any order, fp64 in a fixed one
#pragma unroll
  for (int i = 0; i < NCNT; ++i) {
    const int v = wave_sum_i(cnt[i]);
    if (lane == 0 && v) atomicAdd(&cnt_s[i], v);
  }
#pragma unroll
  for (int i = 0; i < NSUM; ++i) {
    const double v = wave_sum_d(sum[i]);
    if (lane == 0) part_s[wave][i] = v;
  }
  __syncthreads();
  if (tid == 0) a.ist[0] += 1;                                     // steps
  if (tid >= 1 && tid <= NCNT) a.ist[tid] += cnt_s[tid - 1];
  if (tid >= 64 && tid < 64 + 2 * BINS) a.ist[HDR + 2 * (size_t)C + (tid - 64)] += hist_s[tid - 64];
  if (tid >= 128 && tid < 128 + NSUM) {
    double t = 0.0;
    for (int w = 0; w < WAVES; ++w) t += part_s[w][tid - 128];
    a.fst[tid - 128] += t;
  }
  if (LDS_CLS)
    for (int c = tid; c < 2 * C; c += THREADS)
      if (cls_s[c]) cls_g[c] += cls_s[c];
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <bool VEC> void launch(const MonArgs& a, hipStream_t s) {
  if (a.C <= LDS_CLASSES) SR_LAUNCH((pl_monitor_kernel<VEC, true>), dim3(1), dim3(THREADS), 0, s, a);
  else SR_LAUNCH((pl_monitor_kernel<VEC, false>), dim3(1), dim3(THREADS), 0, s, a);
}

}  // namespace

extern "C" int srhip_pl_monitor(const long long* pseudo, const float* mask0, const float* mask_kept, const float* mask2, const float* reward,
                                const long long* idx_ulb, const long long* ulb_targets, long long n_ulb, int P, int nu, int C,
                                long long* istate, double* fstate, void* stream) {
  if (!pseudo || !mask0 || !mask_kept || !idx_ulb || !ulb_targets || !istate || !fstate) return SR_EINVAL;
  if (P <= 0 || nu <= 0 || C <= 0 || n_ulb <= 0) return SR_EINVAL;
  if (P > 1 && (!mask2 || !reward)) return SR_EINVAL;
  if ((long long)P * nu > 0x7fffffffll || C > (1 << 28)) return SR_EINVAL;         // per-launch counters are 32-bit
  if (((uintptr_t)istate & 7u) || ((uintptr_t)fstate & 7u) || ((uintptr_t)pseudo & 7u) || ((uintptr_t)idx_ulb & 7u) ||
      ((uintptr_t)ulb_targets & 7u))
    return SR_EINVAL;
  int* err = sr_label_err_ptr();
  if (!err) return SR_ELAUNCH;
  const MonArgs a{pseudo, mask0, mask_kept, mask2, reward, idx_ulb, ulb_targets, istate, fstate, err, n_ulb, P - 1, nu, C};
  if (P > 1 && al16(reward) && al16(mask2)) launch<true>(a, (hipStream_t)stream);
  else launch<false>(a, (hipStream_t)stream);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
