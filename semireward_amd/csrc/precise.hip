// Split-bf16 ("bf16x3") products for the rows whose outputs decide the pseudo-label masks (read_rows_precision = bf16x3).
//
// Every fp32 operand x is split once into two bf16 planes, hi = bf16_rne(x) and lo = bf16_rne(x - hi) (x - hi is exact in fp32), and a
// product a . b is taken as hi_a . hi_b + hi_a . lo_b + lo_a . hi_b on the bf16 MFMA with one fp32 accumulator (the lo . lo term, ~2^-16
// relative, is dropped).  Three 16x16x32 bf16 MFMAs per fragment pair: 3/16 of the bf16 rate is still ~3x the rate of the exact f32-input
// MFMA (v_mfma_f32_16x16x4_f32), and the error (~4e-6 relative, K up to 3072) is three orders below the bf16-operand path's.
//
//   gemm_nt_x3_kernel  C[M,N] = A[M,K] . W[N,K]^T, fp32 A and W (W straight from the fp32 parameter block), three epilogues:
//                      fp32 + bias (qkv, patch embedding), exact-erf GELU (fc1), residual x += row_scale * (acc + bias) (proj, fc2)
//   attn_fwd_x3_kernel softmax(Q K^T * scale) V per (image, head), head_dim 64, N <= 512, fp32 qkv in / fp32 out; fp32 softmax with
//                      accurate expf, the row sum over the unrounded probabilities
// Reference call sites: semilearn/nets/vit/vit.py:93-105 (qkv, attention, proj), :69-75 (fc1, fc2), :39-44 (patch embedding).
#include "common.h"
#include "srhip.h"
#include "x3.h"

namespace {

// ---------------------------------------------------------------------------------------------
// GEMM: 128 x 128 tile per workgroup, 4 waves in 2 x 2, each 64 x 64 = 4 x 4 fragments; K in steps of 32.  The fp32 tiles of the next step
// are loaded into registers while the current one is multiplied; they are split into hi / lo bf16 planes on their way into LDS.
// LDS rows are 32 bf16 + 8 padding (80 bytes): the 16-byte fragment reads of 8 consecutive rows hit disjoint banks.
constexpr int X3_T = 128, X3_BK = 32, X3_PITCH = 40;

template <int EPI>
__global__ __launch_bounds__(256) void gemm_nt_x3_kernel(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw,
                                                        float* __restrict__ C, int ldc, int M, int N, int K, const float* __restrict__ bias,
                                                        const float* __restrict__ row_scale, int rows_per_sample) {
  __shared__ __attribute__((aligned(16))) bf16_t sm[4][X3_T * X3_PITCH];      // A hi, A lo, W hi, W lo
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.y * X3_T, n0 = blockIdx.x * X3_T;
  // staging map: thread -> rows sr + 32 i (i = 0..3), columns sk .. sk + 3 of the 32-wide K slice (8 threads cover a 128-byte row)
  const int sr = tid >> 3, sk = (tid & 7) * 4;
  const float* ap = A + (size_t)min(m0 + sr, M - 1) * lda + sk;      // rows past M / N read the last row (results discarded)
  const float* wp = W + (size_t)min(n0 + sr, N - 1) * ldw + sk;
  size_t astep[4], wstep[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    astep[i] = (size_t)(min(m0 + sr + 32 * i, M - 1) - min(m0 + sr, M - 1)) * lda;
    wstep[i] = (size_t)(min(n0 + sr + 32 * i, N - 1) - min(n0 + sr, N - 1)) * ldw;
  }
  float4 ra[4], rw[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ra[i] = *reinterpret_cast<const float4*>(ap + astep[i]);
    rw[i] = *reinterpret_cast<const float4*>(wp + wstep[i]);
  }
  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  for (int k0 = 0; k0 < K; k0 += X3_BK) {
    __syncthreads();                                   // the previous step's fragment reads are done
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = (sr + 32 * i) * X3_PITCH + sk;
      uint32_t h0, l0, h1, l1;
      split2(ra[i].x, ra[i].y, h0, l0);
      split2(ra[i].z, ra[i].w, h1, l1);
      *reinterpret_cast<u32x2_t*>(&sm[0][o]) = u32x2_t{h0, h1};
      *reinterpret_cast<u32x2_t*>(&sm[1][o]) = u32x2_t{l0, l1};
      split2(rw[i].x, rw[i].y, h0, l0);
      split2(rw[i].z, rw[i].w, h1, l1);
      *reinterpret_cast<u32x2_t*>(&sm[2][o]) = u32x2_t{h0, h1};
      *reinterpret_cast<u32x2_t*>(&sm[3][o]) = u32x2_t{l0, l1};
    }
    __syncthreads();
    if (k0 + X3_BK < K) {                              // next slice in flight under this step's MFMAs
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        ra[i] = *reinterpret_cast<const float4*>(ap + astep[i] + k0 + X3_BK);
        rw[i] = *reinterpret_cast<const float4*>(wp + wstep[i] + k0 + X3_BK);
      }
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
  // epilogue: fragment (i, j) register r is C[wm + 16 i + 4 g + r][wn + 16 j + l15]
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = n0 + wn + j * 16 + l15;
    if (n >= N) continue;
    const float bn = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + i * 16 + 4 * g + r;
        if (m >= M) continue;
        float* c = C + (size_t)m * ldc + n;
        const float v = acc[i][j][r] + bn;
        if constexpr (EPI == SRHIP_X3_EPI_F32) {
          *c = v;
        } else if constexpr (EPI == SRHIP_X3_EPI_GELU_F32) {
          *c = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));      // nn.GELU(), exact erf (vit.py:63,72)
        } else {
          const float s = row_scale ? row_scale[m / rows_per_sample] : 1.0f;
          *c = *c + s * v;                                                      // DropPath + residual (vit.py:164-165)
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Attention: one wave = 16 queries of one (image, head), four waves per workgroup.  The scores are taken transposed, S^T = K Q^T (keys on
// the accumulator rows, the query on the lane), so that the probabilities of a 32-key step are the B operand of O^T = V^T P^T in place:
// lane (g, q) holds keys 4 g + r and 16 + 4 g + r (r = 0..3) of its query, and the V^T fragment is gathered in that key order.
// Two passes over the keys: the exact row maximum first, then exp, the row sum and P V -- the softmax is evaluated as
// exp(s - max) / sum(exp) in fp32 as torch.softmax does, no running rescale.
__global__ __launch_bounds__(256) void attn_fwd_x3_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int H, float scale) {
  attn_fwd_x3_wave<false>(qkv, out, N, H, scale, nullptr);
}

}  // namespace

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int srhip_gemm_nt_x3(int epilogue, const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                                const float* bias, const float* row_scale, int rows_per_sample, void* stream) {
  if (!A || !W || !C || M <= 0 || N <= 0 || K <= 0 || K % X3_BK || lda < K || ldw < K || ldc < N || lda % 4 || ldw % 4 ||
      !aligned16(A) || !aligned16(W) || (row_scale && rows_per_sample <= 0) || (row_scale && epilogue != SRHIP_X3_EPI_RESID_F32) ||
      cdiv(M, X3_T) > 65535)
    return SR_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(cdiv(N, X3_T), cdiv(M, X3_T)), block(256);
  switch (epilogue) {
    case SRHIP_X3_EPI_F32:
      SR_LAUNCH(gemm_nt_x3_kernel<SRHIP_X3_EPI_F32>, grid, block, 0, s, A, lda, W, ldw, C, ldc, M, N, K, bias, row_scale, rows_per_sample);
      break;
    case SRHIP_X3_EPI_GELU_F32:
      SR_LAUNCH(gemm_nt_x3_kernel<SRHIP_X3_EPI_GELU_F32>, grid, block, 0, s, A, lda, W, ldw, C, ldc, M, N, K, bias, row_scale, rows_per_sample);
      break;
    case SRHIP_X3_EPI_RESID_F32:
      SR_LAUNCH(gemm_nt_x3_kernel<SRHIP_X3_EPI_RESID_F32>, grid, block, 0, s, A, lda, W, ldw, C, ldc, M, N, K, bias, row_scale, rows_per_sample);
      break;
    default:
      return SR_EINVAL;
  }
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_attn_fwd_x3(const float* qkv, float* out, int B, int N, int H, float scale, void* stream) {
  if (!qkv || !out || B <= 0 || N <= 0 || N > 512 || H <= 0 || B > 65535 || !aligned16(qkv) || !aligned16(out)) return SR_EINVAL;
  SR_LAUNCH(attn_fwd_x3_kernel, dim3(cdiv(N, 64), H, B), dim3(256), 0, (hipStream_t)stream, qkv, out, N, H, scale);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
