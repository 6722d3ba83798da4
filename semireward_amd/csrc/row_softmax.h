// The row-softmax body shared by the one-wave-per-row kernels that must agree bit for bit on (max probability, argmax): srhip_row_max
// (score_filter.hip) and srhip_score_rows (score_rows.hip).
//
// A row's columns are owned by the lanes in ONE layout -- lane l owns columns l, l + 64, l + 128, ... -- and a kernel hands the body a
// `sweep`: a callable that visits the calling lane's columns in ascending order, sweep(g) -> g(c, z_c).  How the logits reach the lane
// (scalar loads, registers filled from a staged row) is the kernel's business; the order of the fp32 operations is fixed here:
//   mx  = max_c z_c                           per-lane fmaxf in column order, then the xor butterfly
//   s   = sum_c expf(z_c - mx)                per-lane sum in column order, then the xor butterfly
//   p_c = expf(z_c - mx) * (1.0f / s)
//   argmax: the largest p_c, the lowest column among equals (torch.max / argmax)
#pragma once
#include "common.h"

// op by op: no fused multiply-add anywhere the two kernels must agree
#pragma clang fp contract(off)

// wave-level (value, index) max with first-index tie break (torch.max / argmax semantics)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
}

// row maximum and the reciprocal of the softmax denominator, the same values in every lane
template <typename Sweep> __device__ __forceinline__ void row_softmax_norm(Sweep&& sweep, float& mx, float& inv) {
  float m = -INFINITY;
  sweep([&](int, float z) { m = fmaxf(m, z); });
  m = wave_max(m);
  float s = 0.f;
  sweep([&](int, float z) { s += expf(z - m); });
  mx = m;
  inv = 1.0f / wave_sum(s);
}

__device__ __forceinline__ float row_softmax_prob(float z, float mx, float inv) { return expf(z - mx) * inv; }
