// Split-bf16 ("bf16x3") kernels: the forward of the rows whose outputs decide the pseudo-label masks (read_rows_precision = bf16x3), the forward
// of the gradient rows that keeps what the backward needs, and that backward (grad_rows_precision = bf16x3).
//
// Every fp32 operand x is split once into two bf16 planes, hi = bf16_rne(x) and lo = bf16_rne(x - hi) (x - hi is exact in fp32), and a
// product a . b is taken as hi_a . hi_b + hi_a . lo_b + lo_a . hi_b on the bf16 MFMA with one fp32 accumulator (the lo . lo term, ~2^-16
// relative, is dropped).  Three 16x16x32 bf16 MFMAs per fragment pair: 3/16 of the bf16 rate is still ~3x the rate of the exact f32-input
// MFMA (v_mfma_f32_16x16x4_f32), and the error (~4e-6 relative, K up to 3072) is three orders below the bf16-operand path's.  fp32 everywhere else.
//
//   gemm_x3_kernel<LA, LB, EPI>  one 128 x 128 tile engine behind srhip_gemm_nt_x3, srhip_gemm_x3 and the grouped launch, three operand layouts:
//       NT  C[M,N] = A[M,K] . B[N,K]^T   (B straight from the fp32 parameter block.  F32: fp32 + bias (qkv, patch embedding); GELU: exact-erf
//                                         GELU (fc1); RESID: x += row_scale * (acc + bias) (proj, fc2); GELU_PRE: fc1 with the pre-activation kept)
//       NN  C[M,N] = A[M,K] . B[K,N]     (input gradients dY . W, W as the parameter block stores it: F32, ACC, DGELU)
//       TN  C[M,N] += A[K,M]^T . B[K,N]  (weight gradients dW += dY^T X over the token axis K, any K: ragged tails are zero-filled; dbias += the
//                                         column sums of A), all problems of a backward in one table-driven launch (srhip_group_tn_desc)
//   attn_fwd_x3_kernel<LSE>      softmax(Q K^T * scale) V per (image, head), head_dim 64, N <= 512, fp32 qkv in / fp32 out; fp32 softmax with
//                                accurate expf, the row sum over the unrounded probabilities.  LSE: also lse = max + log(sum) for the backward
//   attn_bwd_x3_dq_kernel        dQ = scale dS K and delta = rowsum(dO o O) per (image, head, 16 queries)
//   attn_bwd_x3_dkv_kernel       dV = P^T dO, dK = scale dS^T Q per (image, head, 16 keys); P = exp(S scale - lse) recomputed, dS = P o (dP - delta)
//   scale_rows_f32_kernel        out = row_scale[m / rows_per_sample] * x (the DropPath factor of the top block's MLP branch)
// Reference call sites: semilearn/nets/vit/vit.py:93-105 (qkv, attention, proj), :69-75 (fc1, GELU, fc2), :39-44 (patch embedding), and their
// autograd.
#include "common.h"
#include "srhip.h"

namespace {

// ---------------------------------------------------------------------------------------------
// The product.  16x16x32 operand lane (g = lane >> 4, l15 = lane & 15) holds row l15, k = 8 g .. 8 g + 7; the result register r of lane
// (g, l15) is C[4 g + r][l15] of C = A . B^T.
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

// ---------------------------------------------------------------------------------------------
// GEMM: 128 x 128 tile per workgroup, 4 waves in 2 x 2, each 64 x 64 = 4 x 4 fragments; K in steps of 32.  The fp32 tiles of the next step
// are loaded into registers while the current one is multiplied; they are split into hi / lo bf16 planes on their way into LDS.
// LDS rows are 32 bf16 + 8 padding (80 bytes): the 16-byte fragment reads of 8 consecutive rows hit disjoint banks.
constexpr int X3_T = 128, X3_BK = 32, X3_PITCH = 40;
enum { LAY_ROWS = 0, LAY_COLS = 1 };     // operand [tile rows][K] (K contiguous) / [K][tile rows] (tile rows contiguous)
// (the public SRHIP_X3_EPI_* and SRHIP_X3B_EPI_* values are mapped onto these by their entry points)
enum { EPI_F32, EPI_ACC, EPI_DGELU, EPI_GELU_PRE, EPI_GELU, EPI_RESID };

struct X3Prob {
  const float* A; const float* B; float* C; const float* bias; const float* aux; float* aux_out; float* colsum; const float* row_scale;
  int lda, ldb, ldc, ldaux, M, N, K, rows_per_sample;
};

// One K slice of an operand tile into registers.  ROWS: thread -> tile rows sr + 32 i, k columns sk .. sk + 3 (8 threads cover a 128-byte
// row; rows past R read row R - 1; results discarded).  COLS: thread -> k rows 2 kr, 2 kr + 1, tile-row quads 4 cq and 64 + 4 cq (quads
// past R and k rows past K read as 0).
template <int LAY>
__device__ __forceinline__ void xb_load(const float* __restrict__ P, int ld, int r0, int R, int k0, int K, float4 (&v)[4]) {
  const int tid = threadIdx.x;
  if constexpr (LAY == LAY_ROWS) {
    const int sr = tid >> 3, sk = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const float4*>(P + (size_t)min(r0 + sr + 32 * i, R - 1) * ld + k0 + sk);
  } else {
    const int kr = tid >> 4, cq = tid & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int k = k0 + 2 * kr + e, c = r0 + 64 * h + 4 * cq;
        v[2 * h + e] = (k < K && c < R) ? *reinterpret_cast<const float4*>(P + (size_t)k * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
  }
}

// registers -> hi / lo planes in LDS, both layouts as [tile row][32 k] (pitch 40)
template <int LAY>
__device__ __forceinline__ void xb_store(const float4 (&v)[4], bf16_t* __restrict__ hi, bf16_t* __restrict__ lo) {
  const int tid = threadIdx.x;
  if constexpr (LAY == LAY_ROWS) {
    const int sr = tid >> 3, sk = (tid & 7) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = (sr + 32 * i) * X3_PITCH + sk;
      uint32_t h0, l0, h1, l1;
      split2(v[i].x, v[i].y, h0, l0);
      split2(v[i].z, v[i].w, h1, l1);
      *reinterpret_cast<u32x2_t*>(&hi[o]) = u32x2_t{h0, h1};
      *reinterpret_cast<u32x2_t*>(&lo[o]) = u32x2_t{l0, l1};
    }
  } else {
    const int kr = tid >> 4, cq = tid & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float a[4] = {v[2 * h].x, v[2 * h].y, v[2 * h].z, v[2 * h].w};
      const float b[4] = {v[2 * h + 1].x, v[2 * h + 1].y, v[2 * h + 1].z, v[2 * h + 1].w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int o = (64 * h + 4 * cq + j) * X3_PITCH + 2 * kr;      // k = 2 kr (low half), 2 kr + 1 (high half)
        uint32_t hh, ll;
        split2(a[j], b[j], hh, ll);
        *reinterpret_cast<uint32_t*>(&hi[o]) = hh;
        *reinterpret_cast<uint32_t*>(&lo[o]) = ll;
      }
    }
  }
}

// nn.GELU(), exact erf (vit.py:63,72)
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }
// d/dx of the exact-erf GELU: Phi(x) + x phi(x)
__device__ __forceinline__ float dgelu_erf(float v) {
  return 0.5f * (1.0f + erff(v * 0.70710678118654752440f)) + v * 0.39894228040143267794f * expf(-0.5f * v * v);
}

template <int LA, int LB, int EPI>
__device__ __forceinline__ void gemm_x3_tile(const X3Prob& p, int tm, int tn, bf16_t (*sm)[X3_T * X3_PITCH]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int m0 = tm * X3_T, n0 = tn * X3_T;
  constexpr bool COLSUM = LA == LAY_COLS;
  const bool do_colsum = COLSUM && p.colsum && tn == 0;
  float4 ra[4], rb[4];
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  xb_load<LA>(p.A, p.lda, m0, p.M, 0, p.K, ra);
  xb_load<LB>(p.B, p.ldb, n0, p.N, 0, p.K, rb);
  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  for (int k0 = 0; k0 < p.K; k0 += X3_BK) {
    __syncthreads();                                   // the previous step's fragment reads are done
    xb_store<LA>(ra, sm[0], sm[1]);
    xb_store<LB>(rb, sm[2], sm[3]);
    if (do_colsum) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        cs[4 * h + 0] += ra[2 * h].x + ra[2 * h + 1].x;
        cs[4 * h + 1] += ra[2 * h].y + ra[2 * h + 1].y;
        cs[4 * h + 2] += ra[2 * h].z + ra[2 * h + 1].z;
        cs[4 * h + 3] += ra[2 * h].w + ra[2 * h + 1].w;
      }
    }
    __syncthreads();
    if (k0 + X3_BK < p.K) {                            // next slice in flight under this step's MFMAs
      xb_load<LA>(p.A, p.lda, m0, p.M, k0 + X3_BK, p.K, ra);
      xb_load<LB>(p.B, p.ldb, n0, p.N, k0 + X3_BK, p.K, rb);
    }
    s16x8_t bh[4], bl[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = (wn + j * 16 + l15) * X3_PITCH + g * 8;
      bh[j] = *reinterpret_cast<const s16x8_t*>(&sm[2][o]);
      bl[j] = *reinterpret_cast<const s16x8_t*>(&sm[3][o]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = (wm + i * 16 + l15) * X3_PITCH + g * 8;
      const s16x8_t ah = *reinterpret_cast<const s16x8_t*>(&sm[0][o]);
      const s16x8_t al = *reinterpret_cast<const s16x8_t*>(&sm[1][o]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma_x3(ah, al, bh[j], bl[j], acc[i][j]);
    }
  }
  if (do_colsum) {                                     // dbias[m] += sum over all K of A[k][m]: 16 partial rows through LDS, fixed order
    __syncthreads();
    float* red = reinterpret_cast<float*>(&sm[0][0]);  // [16][128] fp32 (8 KB of the 40 KB)
    const int kr = tid >> 4, cq = tid & 15;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int j = 0; j < 4; ++j) red[kr * X3_T + 64 * h + 4 * cq + j] = cs[4 * h + j];
    __syncthreads();
    if (tid < X3_T && m0 + tid < p.M) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += red[r * X3_T + tid];
      p.colsum[m0 + tid] += s;
    }
  }
  // epilogue: fragment (i, j) register r is C[wm + 16 i + 4 g + r][wn + 16 j + l15]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn + j * 16 + l15;
    if (n >= p.N) continue;
    const float bn = (EPI != EPI_ACC && EPI != EPI_DGELU) && p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + i * 16 + 4 * g + r;
        if (m >= p.M) continue;
        float* c = p.C + (size_t)m * p.ldc + n;
        const float v = acc[i][j][r] + bn;
        if constexpr (EPI == EPI_F32) {
          *c = v;
        } else if constexpr (EPI == EPI_ACC) {
          *c = *c + v;
        } else if constexpr (EPI == EPI_DGELU) {
          *c = v * dgelu_erf(p.aux[(size_t)m * p.ldaux + n]);
        } else if constexpr (EPI == EPI_GELU_PRE) {    // the fp32 pre-activation for the backward, then nn.GELU()
          p.aux_out[(size_t)m * p.ldaux + n] = v;
          *c = gelu_erf(v);
        } else if constexpr (EPI == EPI_GELU) {
          *c = gelu_erf(v);
        } else {
          const float s = p.row_scale ? p.row_scale[m / p.rows_per_sample] : 1.0f;
          *c = *c + s * v;                                                      // DropPath + residual (vit.py:164-165)
        }
      }
    }
  }
}

template <int LA, int LB, int EPI>
__global__ __launch_bounds__(256) void gemm_x3_kernel(const X3Prob p) {
  __shared__ __attribute__((aligned(16))) bf16_t sm[4][X3_T * X3_PITCH];      // A hi, A lo, B hi, B lo
  gemm_x3_tile<LA, LB, EPI>(p, blockIdx.y, blockIdx.x, sm);
}

// weight gradients: one workgroup per 128 x 128 tile of any problem of the table (tile_start ascending)
__global__ __launch_bounds__(256) void gemm_tn_x3_grouped_kernel(const srhip_group_tn_desc* __restrict__ desc, int n) {
  __shared__ __attribute__((aligned(16))) bf16_t sm[4][X3_T * X3_PITCH];
  const int t = blockIdx.x;
  int i = 0;
  while (i + 1 < n && desc[i + 1].tile_start <= t) ++i;
  const srhip_group_tn_desc d = desc[i];
  X3Prob p = {(const float*)d.A, (const float*)d.B, d.C, nullptr, nullptr, nullptr, d.dbias, nullptr, d.lda, d.ldb, d.ldc, 0, d.M, d.N, d.K, 0};
  const int tiles_n = (d.N + X3_T - 1) / X3_T, local = t - d.tile_start;
  gemm_x3_tile<LAY_COLS, LAY_COLS, EPI_ACC>(p, local / tiles_n, local % tiles_n, sm);
}

// ---------------------------------------------------------------------------------------------
// Attention, head_dim 64: one wave = 16 rows of one (image, head), four waves per workgroup.  A score block is taken transposed (the other
// side's rows on the accumulator rows, the wave's own row on the lane): a 32-wide step's two 16 x 16 blocks leave lane (g, l15) holding the
// entries 4 g + r and 16 + 4 g + r (r = 0..3) of its column l15, which is the B-operand order of the next product -- the A operand is
// gathered in that same order.

// A . B^T of 16 rows of A (from row, clamped to the last valid row) and 16 rows of B, both [., 64] fp32, A at row stride ld: lane (g, l15)
// gets C[4 g + r][l15].
__device__ __forceinline__ f32x4_t dot_x3(const float* __restrict__ abase, int ld, int row, int nrows, int g, const s16x8_t (&bh)[2],
                                          const s16x8_t (&bl)[2]) {
  const float* ap = abase + (size_t)min(row, nrows - 1) * ld + g * 8;
  f32x4_t s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(ap + 32 * t), b = *reinterpret_cast<const float4*>(ap + 32 * t + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    s16x8_t h, l;
    split8(v, h, l);
    s = mfma_x3(h, l, bh[t], bl[t], s);
  }
  return s;
}

// the B-operand planes of one 64-wide row (the caller clamps the row index): lane (g, row) holds dims 32 t + 8 g + j
__device__ __forceinline__ void row_planes(const float* __restrict__ base, int ld, int row, int g, s16x8_t (&h)[2], s16x8_t (&l)[2]) {
  const float* p = base + (size_t)row * ld + g * 8;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float4 a = *reinterpret_cast<const float4*>(p + 32 * t), c = *reinterpret_cast<const float4*>(p + 32 * t + 4);
    const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    split8(v, h[t], l[t]);
  }
}

// Forward: S^T = K Q^T, so that the probabilities of a 32-key step are the B operand of O^T = V^T P^T in place, the V^T fragment gathered in
// that key order.  Two passes over the keys: the exact row maximum first, then exp, the row sum and P V -- the softmax is evaluated as
// exp(s - max) / sum(exp) in fp32 as torch.softmax does, no running rescale.  LSE: also write lse[b][h][q] = max + log(sum).
template <bool LSE>
__global__ __launch_bounds__(256) void attn_fwd_x3_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int H, float scale,
                                                         float* __restrict__ lse) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, q0 = (blockIdx.x * 4 + wave) * 16;
  if (q0 >= N) return;                                 // (no workgroup barrier in this kernel)
  const int D = H * 64, ld = 3 * D;
  const float* base = qkv + (size_t)b * N * ld + h * 64;
  const float* kbase = base + D;
  const float* vbase = base + 2 * D;
  s16x8_t qh[2], ql[2];
  row_planes(base, ld, min(q0 + l15, N - 1), g, qh, ql);
  float mx = -INFINITY;
  for (int kb = 0; kb < N; kb += 16) {
    const f32x4_t s = dot_x3(kbase, ld, kb + l15, N, g, qh, ql);
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
    const f32x4_t s0 = dot_x3(kbase, ld, kb + l15, N, g, qh, ql);
    const f32x4_t s1 = dot_x3(kbase, ld, kb + 16 + l15, N, g, qh, ql);
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

__global__ __launch_bounds__(256) void attn_bwd_x3_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                            const float* __restrict__ dout, const float* __restrict__ lse,
                                                            float* __restrict__ dqkv, float* __restrict__ delta, int N, int H, float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, q0 = (blockIdx.x * 4 + wave) * 16;
  if (q0 >= N) return;                                 // (no workgroup barrier in this kernel)
  const int D = H * 64, ld = 3 * D;
  const float* base = qkv + (size_t)b * N * ld + h * 64;
  const float* kbase = base + D;
  const float* vbase = base + 2 * D;
  const float* obase = o + (size_t)b * N * D + h * 64;
  const float* dobase = dout + (size_t)b * N * D + h * 64;
  const int q = min(q0 + l15, N - 1);
  s16x8_t qh[2], ql[2], dh[2], dl[2];
  row_planes(base, ld, q, g, qh, ql);
  row_planes(dobase, D, q, g, dh, dl);
  // delta[q] = sum_d dO[q][d] O[q][d] in fp32: lane (g, q) holds the dims 32 t + 8 g + j
  float dsum = 0.f;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int d = 32 * t + 8 * g + j;
      dsum += dobase[(size_t)q * D + d] * obase[(size_t)q * D + d];
    }
  dsum += __shfl_xor(dsum, 16, 64);
  dsum += __shfl_xor(dsum, 32, 64);
  const size_t srow = ((size_t)b * H + h) * N;
  if (g == 0 && q0 + l15 < N) delta[srow + q] = dsum;
  const float lq = lse[srow + q];
  f32x4_t dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < N; kb += 32) {
    const f32x4_t s0 = dot_x3(kbase, ld, kb + l15, N, g, qh, ql), s1 = dot_x3(kbase, ld, kb + 16 + l15, N, g, qh, ql);      // S^T
    const f32x4_t p0 = dot_x3(vbase, ld, kb + l15, N, g, dh, dl), p1 = dot_x3(vbase, ld, kb + 16 + l15, N, g, dh, dl);      // dP^T = V dO^T
    float ds[8];
    int key[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      key[r] = kb + 4 * g + r;
      key[4 + r] = kb + 16 + 4 * g + r;
      ds[r] = key[r] < N ? expf(s0[r] * scale - lq) * (p0[r] - dsum) : 0.f;
      ds[4 + r] = key[4 + r] < N ? expf(s1[r] * scale - lq) * (p1[r] - dsum) : 0.f;
    }
    s16x8_t sh, sl;
    split8(ds, sh, sl);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      float kv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kv[j] = kbase[(size_t)min(key[j], N - 1) * ld + dt * 16 + l15];
      s16x8_t kh, kl;
      split8(kv, kh, kl);
      dq[dt] = mfma_x3(kh, kl, sh, sl, dq[dt]);        // dQ^T[dim dt 16 + 4 g + r][query l15]
    }
  }
  if (q0 + l15 >= N) return;
  float* op = dqkv + ((size_t)b * N + q) * ld + h * 64 + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<float4*>(op + dt * 16) = make_float4(dq[dt][0] * scale, dq[dt][1] * scale, dq[dt][2] * scale, dq[dt][3] * scale);
}

__global__ __launch_bounds__(256) void attn_bwd_x3_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                             const float* __restrict__ lse, const float* __restrict__ delta,
                                                             float* __restrict__ dqkv, int N, int H, float scale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, k0 = (blockIdx.x * 4 + wave) * 16;
  if (k0 >= N) return;
  const int D = H * 64, ld = 3 * D;
  const float* base = qkv + (size_t)b * N * ld + h * 64;
  const float* kbase = base + D;
  const float* vbase = base + 2 * D;
  const float* dobase = dout + (size_t)b * N * D + h * 64;
  const size_t srow = ((size_t)b * H + h) * N;
  const int key = min(k0 + l15, N - 1);
  s16x8_t kh[2], kl[2], vh[2], vl[2];
  row_planes(kbase, ld, key, g, kh, kl);
  row_planes(vbase, ld, key, g, vh, vl);
  f32x4_t dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dk[dt] = dv[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int qb = 0; qb < N; qb += 32) {
    const f32x4_t s0 = dot_x3(base, ld, qb + l15, N, g, kh, kl), s1 = dot_x3(base, ld, qb + 16 + l15, N, g, kh, kl);       // S[q][key]
    const f32x4_t p0 = dot_x3(dobase, D, qb + l15, N, g, vh, vl), p1 = dot_x3(dobase, D, qb + 16 + l15, N, g, vh, vl);     // dP[q][key]
    float pr[8], ds[8];
    int qr[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      qr[r] = qb + 4 * g + r;
      qr[4 + r] = qb + 16 + 4 * g + r;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int qc = min(qr[j], N - 1);
      const float s = j < 4 ? s0[j] : s1[j - 4], dp = j < 4 ? p0[j] : p1[j - 4];
      pr[j] = qr[j] < N ? expf(s * scale - lse[srow + qc]) : 0.f;
      ds[j] = pr[j] * (dp - delta[srow + qc]);
      qr[j] = qc;
    }
    s16x8_t ph, pl, sh, sl;
    split8(pr, ph, pl);
    split8(ds, sh, sl);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      float dov[8], qv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dov[j] = dobase[(size_t)qr[j] * D + dt * 16 + l15];
        qv[j] = base[(size_t)qr[j] * ld + dt * 16 + l15];
      }
      s16x8_t ah, al;
      split8(dov, ah, al);
      dv[dt] = mfma_x3(ah, al, ph, pl, dv[dt]);        // dV^T[dim][key l15]
      split8(qv, ah, al);
      dk[dt] = mfma_x3(ah, al, sh, sl, dk[dt]);        // dK^T[dim][key l15] / scale
    }
  }
  if (k0 + l15 >= N) return;
  float* op = dqkv + ((size_t)b * N + key) * ld + h * 64 + 4 * g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    *reinterpret_cast<float4*>(op + D + dt * 16) = make_float4(dk[dt][0] * scale, dk[dt][1] * scale, dk[dt][2] * scale, dk[dt][3] * scale);
    *reinterpret_cast<float4*>(op + 2 * D + dt * 16) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
  }
}

__global__ void scale_rows_f32_kernel(const float* __restrict__ x, const float* __restrict__ scale, int rows_per_sample, float* __restrict__ out,
                                      size_t n4, int D) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  const float s = scale ? scale[(i * 4 / D) / rows_per_sample] : 1.0f;
  const float4 a = reinterpret_cast<const float4*>(x)[i];
  reinterpret_cast<float4*>(out)[i] = make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int LA, int LB, int EPI>
void launch_x3(const X3Prob& p, hipStream_t s) {
  SR_LAUNCH((gemm_x3_kernel<LA, LB, EPI>), dim3(cdiv(p.N, X3_T), cdiv(p.M, X3_T)), dim3(256), 0, s, p);
}

}  // namespace

extern "C" int srhip_gemm_nt_x3(int epilogue, const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                                const float* bias, const float* row_scale, int rows_per_sample, void* stream) {
  if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0 || K % X3_BK || lda < K || ldw < K || ldc < N || lda % 4 || ldw % 4 ||
      !aligned16(A) || !aligned16(W) || (row_scale && rows_per_sample <= 0) || (row_scale && epilogue != SRHIP_X3_EPI_RESID_F32) ||
      cdiv(M, X3_T) > 65535)
    return SR_EINVAL;
  const X3Prob p = {A, W, C, bias, nullptr, nullptr, nullptr, row_scale, lda, ldw, ldc, 0, M, N, K, rows_per_sample};
  hipStream_t s = (hipStream_t)stream;
  switch (epilogue) {
    case SRHIP_X3_EPI_F32: launch_x3<LAY_ROWS, LAY_ROWS, EPI_F32>(p, s); break;
    case SRHIP_X3_EPI_GELU_F32: launch_x3<LAY_ROWS, LAY_ROWS, EPI_GELU>(p, s); break;
    case SRHIP_X3_EPI_RESID_F32: launch_x3<LAY_ROWS, LAY_ROWS, EPI_RESID>(p, s); break;
    default: return SR_EINVAL;
  }
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_gemm_x3(int layout, int epilogue, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                             const float* bias, const float* aux, float* aux_out, int ldaux, void* stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || K % X3_BK || lda % 4 || ldb % 4 || ldc < N || !aligned16(A) || !aligned16(B) ||
      cdiv(M, X3_T) > 65535)
    return SR_EINVAL;
  const X3Prob p = {A, B, C, bias, aux, aux_out, nullptr, nullptr, lda, ldb, ldc, ldaux, M, N, K, 0};
  hipStream_t s = (hipStream_t)stream;
  if (layout == SRHIP_X3B_NT) {
    if (epilogue != SRHIP_X3B_EPI_GELU_PRE || !aux_out || ldaux < N || lda < K || ldb < K) return SR_EINVAL;
    launch_x3<LAY_ROWS, LAY_ROWS, EPI_GELU_PRE>(p, s);
  } else if (layout == SRHIP_X3B_NN) {
    if (lda < K || ldb < N || N % 4 || bias) return SR_EINVAL;
    switch (epilogue) {
      case SRHIP_X3B_EPI_F32: launch_x3<LAY_ROWS, LAY_COLS, EPI_F32>(p, s); break;
      case SRHIP_X3B_EPI_ACC: launch_x3<LAY_ROWS, LAY_COLS, EPI_ACC>(p, s); break;
      case SRHIP_X3B_EPI_DGELU:
        if (!aux || ldaux < N) return SR_EINVAL;
        launch_x3<LAY_ROWS, LAY_COLS, EPI_DGELU>(p, s);
        break;
      default: return SR_EINVAL;
    }
  } else {
    return SR_EINVAL;
  }
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_gemm_tn_x3_grouped(const srhip_group_tn_desc* desc_dev, int n_problems, int total_tiles, void* stream) {
  if (!desc_dev || n_problems <= 0 || total_tiles <= 0) return SR_EINVAL;
  SR_LAUNCH(gemm_tn_x3_grouped_kernel, dim3(total_tiles), dim3(256), 0, (hipStream_t)stream, desc_dev, n_problems);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_attn_fwd_x3(const float* qkv, float* out, int B, int N, int H, float scale, void* stream) {
  if (!qkv || !out || B <= 0 || N <= 0 || N > 512 || H <= 0 || B > 65535 || !aligned16(qkv) || !aligned16(out)) return SR_EINVAL;
  SR_LAUNCH(attn_fwd_x3_kernel<false>, dim3(cdiv(N, 64), H, B), dim3(256), 0, (hipStream_t)stream, qkv, out, N, H, scale, (float*)nullptr);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_attn_fwd_x3_lse(const float* qkv, float* out, float* lse, int B, int N, int H, float scale, void* stream) {
  if (!qkv || !out || !lse || B <= 0 || N <= 0 || N > 512 || H <= 0 || B > 65535 || !aligned16(qkv) || !aligned16(out)) return SR_EINVAL;
  SR_LAUNCH(attn_fwd_x3_kernel<true>, dim3(cdiv(N, 64), H, B), dim3(256), 0, (hipStream_t)stream, qkv, out, N, H, scale, lse);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_attn_bwd_x3(const float* qkv, const float* out, const float* d_out, const float* lse, float* dqkv, float* delta_ws,
                                 int B, int N, int H, float scale, void* stream) {
  if (!qkv || !out || !d_out || !lse || !dqkv || !delta_ws || B <= 0 || N <= 0 || N > 512 || H <= 0 || B > 65535 || !aligned16(qkv) ||
      !aligned16(out) || !aligned16(d_out) || !aligned16(dqkv))
    return SR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(N, 64), H, B);
  SR_LAUNCH(attn_bwd_x3_dq_kernel, grid, dim3(256), 0, s, qkv, out, d_out, lse, dqkv, delta_ws, N, H, scale);
  SR_CHECK_LAUNCH();
  SR_LAUNCH(attn_bwd_x3_dkv_kernel, grid, dim3(256), 0, s, qkv, d_out, lse, delta_ws, dqkv, N, H, scale);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_scale_rows_f32(const float* x, const float* scale, int rows_per_sample, float* out, long M, int D, void* stream) {
  if (!x || !out || M <= 0 || D % 4 || (scale && rows_per_sample <= 0) || !aligned16(x) || !aligned16(out)) return SR_EINVAL;
  const size_t n4 = (size_t)M * D / 4;
  SR_LAUNCH(scale_rows_f32_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, x, scale, rows_per_sample > 0 ? rows_per_sample : 1,
            out, n4, D);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
