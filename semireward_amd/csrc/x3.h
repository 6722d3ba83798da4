// Split-bf16 ("bf16x3") product helpers shared by csrc/precise.hip (forward) and csrc/precise_bwd.hip (backward).
// x = hi + lo with hi = bf16_rne(x), lo = bf16_rne(x - hi); a . b ~ hi_a . hi_b + hi_a . lo_b + lo_a . hi_b, three 16x16x32 bf16 MFMAs into one
// fp32 accumulator.  16x16x32 operand lane (g = lane >> 4, l15 = lane & 15) holds row l15, k = 8 g .. 8 g + 7; the result register r of lane
// (g, l15) is C[4 g + r][l15] of C = A . B^T.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ f32x4_t mfma_x(const s16x8_t a, const s16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
}

// hi / lo planes of two fp32 values, packed as two bf16 each (element order kept)
__device__ __forceinline__ void split2(float x, float y, uint32_t& hi, uint32_t& lo) {
  hi = pack_bf2(x, y);
  lo = pack_bf2(x - __uint_as_float(hi << 16), y - __uint_as_float(hi & 0xffff0000u));
}

// eight fp32 values -> the hi and lo fragments of one 16x16x32 operand lane
__device__ __forceinline__ void split8(const float (&v)[8], s16x8_t& hi, s16x8_t& lo) {
  u32x4_t h, l;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t a, b;
    split2(v[2 * i], v[2 * i + 1], a, b);
    h[i] = a;
    l[i] = b;
  }
  hi = __builtin_bit_cast(s16x8_t, h);
  lo = __builtin_bit_cast(s16x8_t, l);
}

__device__ __forceinline__ f32x4_t mfma_x3(const s16x8_t ah, const s16x8_t al, const s16x8_t bh, const s16x8_t bl, f32x4_t c) {
  c = mfma_x(ah, bl, c);
  c = mfma_x(al, bh, c);
  return mfma_x(ah, bh, c);
}

__device__ __forceinline__ f32x4_t score_x3(const float* __restrict__ kbase, int ld, int key, int N, int g, const s16x8_t (&qh)[2],
                                            const s16x8_t (&ql)[2]) {
  const float* kp = kbase + (size_t)min(key, N - 1) * ld + g * 8;
  f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(kp + 32 * t), b = *reinterpret_cast<const float4*>(kp + 32 * t + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    s16x8_t kh, kl;
    split8(v, kh, kl);
    s = mfma_x3(kh, kl, qh[t], ql[t], s);
  }
  return s;
}

// The attention forward of one wave (attn_fwd_x3_kernel, csrc/precise.hip).  LSE: also write lse[b][h][q] = max + log(sum), the softmax
// statistic of the backward (attn_fwd_x3_lse_kernel, csrc/precise_bwd.hip).
template <bool LSE>
__device__ __forceinline__ void attn_fwd_x3_wave(const float* __restrict__ qkv, float* __restrict__ out, int N, int H, float scale,
                                                 float* __restrict__ lse) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, q0 = (blockIdx.x * 4 + wave) * 16;
  if (q0 >= N) return;                                 // (no workgroup barrier in this kernel)
  const int D = H * 64, ld = 3 * D;
  const float* base = qkv + (size_t)b * N * ld + h * 64;
  const float* kbase = base + D;
  const float* vbase = base + 2 * D;
  // Q as the B operand of S^T: lane (g, q) holds Q[q][32 t + 8 g + j]
  s16x8_t qh[2], ql[2];
  {
    const float* qp = base + (size_t)min(q0 + l15, N - 1) * ld + g * 8;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 a = *reinterpret_cast<const float4*>(qp + 32 * t), c = *reinterpret_cast<const float4*>(qp + 32 * t + 4);
      const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
      split8(v, qh[t], ql[t]);
    }
  }
  float mx = -INFINITY;
  for (int kb = 0; kb < N; kb += 16) {
    const f32x4_t s = score_x3(kbase, ld, kb + l15, N, g, qh, ql);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (kb + 4 * g + r < N) mx = fmaxf(mx, s[r] * scale);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  f32x4_t o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float l = 0.f;
  for (int kb = 0; kb < N; kb += 32) {
    const f32x4_t s0 = score_x3(kbase, ld, kb + l15, N, g, qh, ql);
    const f32x4_t s1 = score_x3(kbase, ld, kb + 16 + l15, N, g, qh, ql);
    float p[8];
    int key[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      key[r] = kb + 4 * g + r;
      key[4 + r] = kb + 16 + 4 * g + r;
      p[r] = key[r] < N ? expf(s0[r] * scale - mx) : 0.f;                // padded keys: probability 0 (as attn_fwd masks them)
      p[4 + r] = key[4 + r] < N ? expf(s1[r] * scale - mx) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) l += p[j];
    s16x8_t ph, pl;
    split8(p, ph, pl);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = vbase[(size_t)min(key[j], N - 1) * ld + dt * 16 + l15];
      s16x8_t vh, vl;
      split8(v, vh, vl);
      o[dt] = mfma_x3(vh, vl, ph, pl, o[dt]);
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const int q = q0 + l15;
  if (q >= N) return;
  const float inv = 1.0f / l;
  if constexpr (LSE) {
    if (g == 0) lse[((size_t)b * H + h) * N + q] = mx + logf(l);
  }
  float* op = out + ((size_t)b * N + q) * D + h * 64 + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<float4*>(op + dt * 16) = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
}

}  // namespace
