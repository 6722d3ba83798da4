// Device bodies of the small "sums over all rows" launches that follow the dX chain of the ViT backward: the LayerNorm partial-copy fold, the
// classifier head's weight / bias gradient, the positional / class-token gradient and stage 1 of the patch-embedding weight gradient.
// Each body takes the workgroup indices and the thread count as arguments, so that the same code runs as a launch of its own (vit_ops.hip) and
// as extra workgroups behind the tiles of the grouped weight-gradient launch (gemm_tn.hip: gemm_tn_grouped_tail_f32_kernel).  One output
// element is always summed by one thread in one fixed order: the two forms give the same bits.
#pragma once
#include "common.h"
#include "srhip.h"

namespace {

constexpr int PE_TOK = 32;     // tokens per workgroup of the small-patch embedding kernels

// dgamma / dbeta of LayerNorm `by` += the sum of its n_rep partial copies ([n_ln][n_rep][2][D]); the copies are cleared for the next step.
// 256 threads; bx < ceil(2 D / 256).
__device__ __forceinline__ void ln_grad_reduce_body(const srhip_ln_reduce_desc* __restrict__ desc, float* __restrict__ part, int n_rep, int D,
                                                    int bx, int by, int tid) {
  const int c = bx * 256 + tid;
  if (c >= 2 * D) return;
  float* p = part + (size_t)by * n_rep * 2 * D + c;
  float acc = 0.f;
  for (int r = 0; r < n_rep; ++r) { acc += p[(size_t)r * 2 * D]; p[(size_t)r * 2 * D] = 0.f; }
  const srhip_ln_reduce_desc d = desc[by];
  float* dst = c < D ? d.dgamma + c : d.dbeta + (c - D);
  *dst += acc;
}

// dWh[c,:] += sum_b dlogits[b,c] * feat[b,:]; dbh[c] += sum_b dlogits[b,c].  256 threads, one workgroup per class c.
__device__ __forceinline__ void cls_head_bwd_w_body(const float* __restrict__ dlogits, const float* __restrict__ feat, float* __restrict__ dWh,
                                                    float* __restrict__ dbh, int B, int D, int C, int c, int tid) {
  for (int d = tid; d < D; d += 256) {
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dlogits[(size_t)b * C + c] * feat[(size_t)b * D + d];
    dWh[(size_t)c * D + d] += a;
  }
  if (tid == 0) {
    float a = 0.f;
    for (int b = 0; b < B; ++b) a += dlogits[(size_t)b * C + c];
    dbh[c] += a;
  }
}

// dpos[t,d] += sum_b dx[b,t,d]; dcls[d] += sum_b dx[b,0,d].  One workgroup per token t, nthr threads over d.
__device__ __forceinline__ void pe_bwd_pos_body(const float* __restrict__ dx, float* __restrict__ dpos, float* __restrict__ dcls, int B, int N,
                                                int D, int t, int tid, int nthr) {
  for (int d = tid; d < D; d += nthr) {
    float s = 0.f;
    for (int b = 0; b < B; ++b) s += dx[((size_t)b * N + t) * D + d];
    dpos[(size_t)t * D + d] += s;
    if (t == 0) dcls[d] += s;
  }
}

// Stage 1 of the atomic-free patch-embed weight gradient: the sums of one (32-token chunk bx, image by) workgroup into ws[by * nbx + bx][k][d]
// (k = K: the bias column).  patch: LDS, PE_TOK * K floats.  nthr threads over d; every thread of the workgroup must call.
__device__ __forceinline__ void pe_bwd_part_body(const float* __restrict__ dx, const float* __restrict__ img, const int* __restrict__ img_index,
                                                 float* __restrict__ ws, int C, int HW, int ps, int D, float* patch, int bx, int by, int nbx,
                                                 int tid, int nthr) {
  const int gw = HW / ps, N = gw * gw + 1, K = C * ps * ps;
  const int b = by, t0 = 1 + bx * PE_TOK;
  const int bi = img_index ? img_index[b] : b;
  const float* im = img + (size_t)bi * C * HW * HW;
  const int nt = min(PE_TOK, N - t0);
  for (int e = tid; e < nt * K; e += nthr) {
    const int tt = e / K, k = e % K, p = t0 + tt - 1, py = p / gw, px = p % gw;
    const int c = k / (ps * ps), i = (k / ps) % ps, j = k % ps;
    patch[e] = im[((size_t)c * HW + py * ps + i) * HW + px * ps + j];
  }
  __syncthreads();
  for (int d = tid; d < D; d += nthr) {
    const float* g0 = dx + ((size_t)b * N + t0) * D + d;
    float* out = ws + (size_t)(by * nbx + bx) * (K + 1) * D + d;
    float accb = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {         // K is small; register-block 16 taps at a time
      float acc[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] = 0.f;
      for (int tb = 0; tb < nt; tb += 8) {       // 8 gradient rows in flight (the loop is otherwise a chain of L2 round trips)
        float g[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) g[i] = (tb + i < nt) ? g0[(size_t)(tb + i) * D] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int tt = min(tb + i, nt - 1);
          if (k0 == 0) accb += g[i];
#pragma unroll
          for (int k = 0; k < 16; ++k)
            if (k0 + k < K) acc[k] += g[i] * patch[tt * K + k0 + k];
        }
      }
#pragma unroll
      for (int k = 0; k < 16; ++k)
        if (k0 + k < K) out[(size_t)(k0 + k) * D] = acc[k];
    }
    out[(size_t)K * D] = accb;
  }
}

}  // namespace
