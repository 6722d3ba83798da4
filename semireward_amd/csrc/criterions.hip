// The rest of the criterion surface (semilearn/core/criterions/cross_entropy.py:11-31, consistency.py:13-45) beside masked_ce_kernel
// (score_filter.hip), which stays the launch of the five shipped algorithms:
//   hard-target cross entropy with reduction none | mean | sum
//   soft-target cross entropy    loss_b = sum_c -t_bc * log_softmax(z_b)_c              (targets NOT assumed to sum to 1)
//   'mse' consistency            loss_b = mean_c (softmax(z_b)_c - t_bc)^2
//   'l1'  consistency            loss_b = mean_c |z_bc - t_bc|
// each times mask_b * mask2_b, with the analytic gradient w.r.t. the logits written by the same launch.
//
// One wave per row.  A row of C <= 1024 logits (and its targets) is read ONCE, with 16-byte loads when base and strides allow, and lives in
// registers (4 x float4 per lane) through the max / sum / gradient sweeps; longer rows are re-read (they hit L2).  All row arithmetic is
// fp32.  The batch reduction has a fixed order and no float atomics, so two runs give the same bits: B <= 64 rows (or no per-row output
// buffer) run as ONE workgroup that finishes the scalar itself -- one launch; larger batches spread one row per wave over the device, write
// the per-row losses, and a one-workgroup kernel adds them (strided per thread, then a fixed tree).  The batch accumulators are fp64: B
// reaches 65 535 and a fixed-order fp32 chain of that length would carry more round-off than the row arithmetic itself.
#include "common.h"
#include "srhip.h"

// op by op, no fused multiply-add: the 16-byte and the scalar instantiations (aligned / unaligned row blocks of one table) must give the same bits
#pragma clang fp contract(off)

namespace {

enum { K_HARD = 0, K_SOFT = 1, K_MSE = 2, K_L1 = 3 };
constexpr int NIT = 4;                    // register-resident chunks: 4 x (64 lanes x 4 floats) = 1024 columns

struct CritArgs {
  const float* logits; long long ld;
  const void* targets; long long ldt;     // K_HARD: int64 [B]; others fp32 [B, C] with row stride ldt
  const float* mask; const float* mask2;
  float grad_scale; int reduction;
  float* loss_rows; float* loss;
  float* dlogits; long long ldd;
  int B, C;
};

// columns c0 .. c0 + 3 of a row; columns >= C read as 0 (every use is guarded by its own c < C test)
template <bool VEC> __device__ __forceinline__ f32x4_t ld4(const float* __restrict__ p, int c0, int C) {
  f32x4_t v = {0.f, 0.f, 0.f, 0.f};
  if (VEC && c0 + 4 <= C) {
    v = *reinterpret_cast<const f32x4_t*>(p + c0);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < C) v[j] = p[c0 + j];
  }
  return v;
}
template <bool VEC> __device__ __forceinline__ void st4(float* __restrict__ p, int c0, int C, f32x4_t v) {
  if (VEC && c0 + 4 <= C) {
    *reinterpret_cast<f32x4_t*>(p + c0) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < C) p[c0 + j] = v[j];
  }
}

template <bool CACHED, typename Fn> __device__ __forceinline__ void each_chunk(int lane, int C, Fn&& f) {
  if constexpr (CACHED) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) f(it, it * 256 + lane * 4);
  } else {
    for (int c0 = lane * 4; c0 < C; c0 += 256) f(0, c0);
  }
}

// Unweighted loss of one row (same value in every lane); the gradient k * d loss / d z is written when dl != NULL.
template <int KIND, bool VEC, bool CACHED>
__device__ __forceinline__ float row_loss_grad(const float* __restrict__ z, const float* __restrict__ t, long long y, float k,
                                               float* __restrict__ dl, int C, int lane) {
  f32x4_t zr[NIT], tr[NIT];
  if constexpr (CACHED) {
    each_chunk<true>(lane, C, [&](int it, int c0) {
      zr[it] = ld4<VEC>(z, c0, C);
      if constexpr (KIND != K_HARD) tr[it] = ld4<VEC>(t, c0, C);
    });
  }
  auto Z = [&](int it, int c0) -> f32x4_t { if constexpr (CACHED) return zr[it]; else return ld4<VEC>(z, c0, C); };
  auto T = [&](int it, int c0) -> f32x4_t { if constexpr (CACHED) return tr[it]; else return ld4<VEC>(t, c0, C); };
  const float invC = 1.0f / (float)C;

  if constexpr (KIND == K_L1) {
    float a = 0.f;
    each_chunk<CACHED>(lane, C, [&](int it, int c0) {
      const f32x4_t zv = Z(it, c0), tv = T(it, c0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) a += fabsf(zv[j] - tv[j]);
    });
    a = wave_sum(a);
    if (dl) {
      const float kc = k * invC;
      each_chunk<CACHED>(lane, C, [&](int it, int c0) {
        const f32x4_t zv = Z(it, c0), tv = T(it, c0);
        f32x4_t g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = zv[j] - tv[j];
          g[j] = d > 0.f ? kc : (d < 0.f ? -kc : 0.f);          // sign(0) = 0, as torch.sign / autograd of l1_loss
        }
        st4<VEC>(dl, c0, C, g);
      });
    }
    return a * invC;
  } else {
    float mx = -INFINITY;
    each_chunk<CACHED>(lane, C, [&](int it, int c0) {
      const f32x4_t zv = Z(it, c0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) mx = fmaxf(mx, zv[j]);
    });
    mx = wave_max(mx);
    float s = 0.f;
    each_chunk<CACHED>(lane, C, [&](int it, int c0) {
      const f32x4_t zv = Z(it, c0);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c0 + j < C) s += expf(zv[j] - mx);
    });
    s = wave_sum(s);
    const float inv = 1.0f / s;

    float loss, g0 = 0.f, g1 = 0.f;      // SOFT: g0 = sum_c t ; MSE: g1 = sum_c p (p - t)
    if constexpr (KIND == K_HARD) {
      const bool ok = y >= 0 && y < (long long)C;               // a label outside [0, C) reads nothing: the row's loss is NaN
      const float zy = ok ? z[y] : NAN;
      loss = logf(s) - (zy - mx);
    } else if constexpr (KIND == K_SOFT) {
      const float ls = logf(s);
      float a = 0.f, ts = 0.f;
      each_chunk<CACHED>(lane, C, [&](int it, int c0) {
        const f32x4_t zv = Z(it, c0), tv = T(it, c0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + j < C) { a += tv[j] * (ls - (zv[j] - mx)); ts += tv[j]; }
      });
      loss = wave_sum(a);
      g0 = wave_sum(ts);
    } else {                                                    // K_MSE
      float a = 0.f, pd = 0.f;
      each_chunk<CACHED>(lane, C, [&](int it, int c0) {
        const f32x4_t zv = Z(it, c0), tv = T(it, c0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (c0 + j < C) {
            const float p = expf(zv[j] - mx) * inv, d = p - tv[j];
            a += d * d;
            pd += p * d;
          }
      });
      loss = wave_sum(a) * invC;
      g1 = wave_sum(pd);
    }
    if (dl) {
      const float k2 = 2.0f * k * invC;
      each_chunk<CACHED>(lane, C, [&](int it, int c0) {
        const f32x4_t zv = Z(it, c0);
        f32x4_t tv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (KIND != K_HARD) tv = T(it, c0);
        f32x4_t g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float p = expf(zv[j] - mx) * inv;
          if constexpr (KIND == K_HARD) g[j] = k * (p - ((long long)(c0 + j) == y ? 1.0f : 0.0f));
          else if constexpr (KIND == K_SOFT) g[j] = k * (p * g0 - tv[j]);
          else g[j] = k2 * p * ((p - tv[j]) - g1);
        }
        st4<VEC>(dl, c0, C, g);
      });
    }
    return loss;
  }
}

// grid = 1: the workgroup walks every row (wave w takes rows w, w + 4, ...) and finishes the scalar; grid = ceil(B / 4): one row per wave,
// per-row losses only (criterion_reduce_kernel adds them).
template <int KIND, bool VEC, bool CACHED> __global__ __launch_bounds__(256) void criterion_kernel(CritArgs a) {
  __shared__ double part[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc = 0.0;
  for (int row = blockIdx.x * 4 + wave; row < a.B; row += gridDim.x * 4) {
    float w = 1.0f;
    if (a.mask) w *= a.mask[row];
    if (a.mask2) w *= a.mask2[row];
    const float k = a.reduction == SRHIP_REDUCE_MEAN ? a.grad_scale * w / (float)a.B : a.grad_scale * w;
    const float* t = KIND == K_HARD ? nullptr : (const float*)a.targets + (size_t)row * a.ldt;
    const long long y = KIND == K_HARD ? ((const long long*)a.targets)[row] : 0;
    const float l = row_loss_grad<KIND, VEC, CACHED>(a.logits + (size_t)row * a.ld, t, y, k,
                                                     a.dlogits ? a.dlogits + (size_t)row * a.ldd : nullptr, a.C, lane) * w;
    if (a.loss_rows && lane == 0) a.loss_rows[row] = l;
    acc += (double)l;
  }
  if (gridDim.x == 1 && a.loss) {
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      const double tot = ((part[0] + part[1]) + part[2]) + part[3];
      a.loss[0] = a.reduction == SRHIP_REDUCE_MEAN ? (float)(tot / (double)a.B) : (float)tot;
    }
  }
}

__global__ __launch_bounds__(1024) void criterion_reduce_kernel(const float* __restrict__ rows, float* __restrict__ loss, int B, int mean) {
  __shared__ double sh[1024];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < B; i += 1024) acc += (double)rows[i];
  sh[tid] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) sh[tid] += sh[tid + o];
    __syncthreads();
  }
  if (tid == 0) loss[0] = mean ? (float)(sh[0] / (double)B) : (float)sh[0];
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int KIND, bool VEC> void launch_kind(const CritArgs& a, int grid, hipStream_t s) {
  if (a.C <= NIT * 256) SR_LAUNCH((criterion_kernel<KIND, VEC, true>), dim3(grid), dim3(256), 0, s, a);
  else SR_LAUNCH((criterion_kernel<KIND, VEC, false>), dim3(grid), dim3(256), 0, s, a);
}

template <int KIND> int criterion(const float* logits, long long ld, const void* targets, long long ldt, const float* mask, const float* mask2,
                                  float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits, long long ldd, int B, int C,
                                  void* stream) {
  if (B <= 0 || C <= 0 || !logits || !targets || ld < C) return SR_EINVAL;
  if (KIND != K_HARD && ldt < C) return SR_EINVAL;
  if (reduction != SRHIP_REDUCE_NONE && reduction != SRHIP_REDUCE_MEAN && reduction != SRHIP_REDUCE_SUM) return SR_EINVAL;
  if (dlogits && ldd < C) return SR_EINVAL;
  if (!loss_rows && !loss && !dlogits) return SR_EINVAL;                       // nothing to compute
  const CritArgs a{logits, ld, targets, ldt, mask, mask2, grad_scale, reduction, loss_rows, loss, dlogits, ldd, B, C};
  const bool vec = al16(logits) && ld % 4 == 0 && (KIND == K_HARD || (al16(targets) && ldt % 4 == 0)) &&
                   (!dlogits || (al16(dlogits) && ldd % 4 == 0));
  const bool one_wg = B <= 64 || (loss && !loss_rows);
  const int grid = one_wg ? 1 : cdiv(B, 4);
  if (vec) launch_kind<KIND, true>(a, grid, (hipStream_t)stream);
  else launch_kind<KIND, false>(a, grid, (hipStream_t)stream);
  SR_CHECK_LAUNCH();
  if (!one_wg && loss) {
    SR_LAUNCH(criterion_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, (const float*)loss_rows, loss, B,
              reduction == SRHIP_REDUCE_MEAN ? 1 : 0);
    SR_CHECK_LAUNCH();
  }
  return SR_OK;
}

}  // namespace

extern "C" int srhip_ce_hard(const float* logits, long long ld, const long long* targets, const float* mask, const float* mask2,
                             float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits, long long ldd, int B, int C,
                             void* stream) {
  return criterion<K_HARD>(logits, ld, targets, 0, mask, mask2, grad_scale, reduction, loss_rows, loss, dlogits, ldd, B, C, stream);
}
extern "C" int srhip_ce_soft(const float* logits, long long ld, const float* targets, long long ldt, const float* mask, const float* mask2,
                             float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits, long long ldd, int B, int C,
                             void* stream) {
  return criterion<K_SOFT>(logits, ld, targets, ldt, mask, mask2, grad_scale, reduction, loss_rows, loss, dlogits, ldd, B, C, stream);
}
extern "C" int srhip_consistency_mse(const float* logits, long long ld, const float* targets, long long ldt, const float* mask,
                                     const float* mask2, float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits,
                                     long long ldd, int B, int C, void* stream) {
  return criterion<K_MSE>(logits, ld, targets, ldt, mask, mask2, grad_scale, reduction, loss_rows, loss, dlogits, ldd, B, C, stream);
}
extern "C" int srhip_consistency_l1(const float* logits, long long ld, const float* targets, long long ldt, const float* mask,
                                    const float* mask2, float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits,
                                    long long ldd, int B, int C, void* stream) {
  return criterion<K_L1>(logits, ld, targets, ldt, mask, mask2, grad_scale, reduction, loss_rows, loss, dlogits, ldd, B, C, stream);
}
