// WideResNet BasicBlock convolution for gfx950 with the BatchNorm around it folded in (semilearn/nets/wrn/wrn.py:41-60):
//
//     y = conv_{k x k, stride}( LeakyReLU(BatchNorm(xin)) ) (+ resid),   and the column statistics of y for the BatchNorm that reads y next
//
// in ONE launch per convolution.  SRPseudoLabel forwards the same 64-image batch K + 1 >= 9 times per step (srpseudolabel.py:59-90); as
// separate kernels a convolution was BN statistics (read y) -> BN apply (read y, write bf16 act) -> im2col (write 9 x act) -> GEMM (read
// 9 x act): ~60 MB of traffic and four launches for a 4 MB activation.  Here:
//   * implicit GEMM: the MFMA B operand (8 consecutive channels of one filter tap of one output pixel) is read straight from the fp32
//     NHWC input -- two 16-byte loads --, normalised + activated in registers with exactly bn_apply_kernel's arithmetic and rounded to
//     bf16 once; padding taps are zeros.  The nine taps of a pixel re-read the input from L1 / L2, not from a materialised col.
//   * the A operand is the filter in the tap-major [Cout, Kpad] bf16 layout of conv_weight_prep, read from L1 / L2 (18-288 KB per layer).
//   * a wave owns 16 output pixels x NT 16-channel tiles (v_mfma_f32_16x16x32_bf16; a lane ends up with 4 consecutive channels of one
//     pixel = one 16-byte store) and walks pixel tiles with a grid stride (<= 512 workgroups); with few pixel tiles and a long K (the
//     16x16 and 8x8 layers) two or four waves of a workgroup share a tile and take every 2nd / 4th k step (LDS reduce).
//   * three k steps are requested ahead of the one being consumed: the loop is bound by the latency of L2 / fabric round trips.
//   * epilogue: + resid, store, and per-channel sum / sum of squares of what was stored: lanes -> wave (shuffles, double from here on)
//     -> workgroup (LDS) -> 16 accumulator copies of the NEXT BatchNorm (fp64 atomics, nobody waits for them).  The launch that reads y
//     folds the copies in its prologue (mode 3), and its workgroup (0, 0) publishes mean / invstd (the backward reads them) and moves the
//     running statistics.  (A fold by the producer's last workgroup -- arrival counter, re-read, store -- was 10-15 us of serial tail.)
//     The caller zeroes the accumulators of all BatchNorms once per forward.
// No LDS staging, no barrier in the main loop: the layers are small (1.2 GFLOP at most) and bound by load latency, which 16 waves per CU
// of independent pixel tiles cover.
#include <stdlib.h>

#include "../../include/srhip.h"
#include "common.h"
#include "wrn_bn.h"

namespace {

struct ConvArgs {
  const float* xin;
  const float* in_mean; const float* in_isd; const float* in_gamma; const float* in_beta;
  const double* in_acc;        // mode 3 (and the publishing workgroup of any mode): accumulator copies [BN_COPIES][2 Cin] of the input BatchNorm
  float in_eps, slope;
  int in_mode;                 // 0: BN(mean, invstd) + LeakyReLU | 1: BN(running mean, running VAR, eps) + LeakyReLU | 2: raw input |
                               // 3: BN(statistics folded from in_acc) + LeakyReLU
  BnFinal pub;                 // pub.out_mean != NULL: workgroup (0, 0) publishes the folded statistics of the input BatchNorm
  const bf16_t* Wb;
  const float* resid;
  float* y;
  int H, W, Cin, log2Cin, Cout, ks, stride, Ho, Wo, Kp, npix, ntiles, in_rows;
  double* acc_out;             // NULL: no statistics; else accumulator copies [BN_COPIES][2 Cout] of the BatchNorm that reads y
  // blockIdx.z = PASS: gridDim.z independent forwards (each its own BatchNorm statistics group, as separate model() calls are in the
  // reference: srpseudolabel.py:59-90 forwards x_ulb_w K + 1 times) share the launch.  Pass-major tensors: xin / y / resid advance by one
  // batch, the accumulators and the published statistics by one BatchNorm's worth; npix, ntiles, in_rows are PER PASS.
  long in_ps, out_ps;          // floats per pass of xin, of y / resid
  // wrn_conv_tile_kernel: one workgroup = one TH x TW block of output pixels of one image (TH * TW = 64 * PG)
  int TW, TH, IW, IH, tiles_x, tiles_y;
  int ipw;                     // images per workgroup (> 1 only when a whole image is one TH x TW block: the 8 x 8 stage takes two)
};

// what a lane requests for one 32-wide k step: its 8 input channels (raw fp32) and NT filter fragments
template <int NT>
struct StepRaw {
  float4 v0, v1;
  u32x4_t af[NT];
  int c;                       // first of the lane's 8 channels; -1: padding / beyond K (B fragment = zeros)
};

template <int NT, int KS>
__global__ __launch_bounds__(256, 2) void wrn_conv_kernel(const ConvArgs a) {
  __shared__ float prm[4][128];                       // mean, invstd, gamma, beta of the input BatchNorm
  __shared__ double redw[4][2][NT * 16];
  __shared__ double red2c[256];
  __shared__ float kred[KS > 1 ? 4 : 1][NT][4][64];    // split K: the partial accumulators of the waves with k part != 0
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int co0 = blockIdx.y * NT * 16, K = a.ks * a.ks * a.Cin, pad = a.ks >> 1, nks = a.Kp >> 5, HoWo = a.Ho * a.Wo;
  const bool stats = a.acc_out != nullptr;
  // this workgroup's pass
  const int ps = blockIdx.z;
  const float* const xin_p = a.xin + (size_t)ps * a.in_ps;
  float* const y_p = a.y + (size_t)ps * a.out_ps;
  const float* const resid_p = a.resid ? a.resid + (size_t)ps * a.out_ps : nullptr;
  const double* const in_acc_p = a.in_acc ? a.in_acc + (size_t)ps * BN_COPIES * 2 * a.Cin : nullptr;
  double* const acc_out_p = a.acc_out ? a.acc_out + (size_t)ps * BN_COPIES * 2 * a.Cout : nullptr;
  BnFinal pub_p = a.pub;
  if (pub_p.out_mean) { pub_p.out_mean += (size_t)ps * a.Cin; pub_p.out_invstd += (size_t)ps * a.Cin; }
  pub_p.update_running = a.pub.update_running && ps == 0;      // (one statistics group moves the running statistics: the caller's first)
  // a lane adds ONE value per pixel tile it walks (<= 4 of them at the launch sizes below): fp32 here, double from the wave reduction on
  float s1[NT][4], s2[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[t][r] = 0.f; s2[t][r] = 0.f; }
  // KS > 1: KS waves of a workgroup share a pixel tile and take every KS-th k step (few pixel tiles, long K: the 16x16 and 8x8 layers run
  // one wave per SIMD otherwise, each walking 18-36 dependent L2 round trips); a workgroup covers 4 / KS tiles per round
  constexpr int TPW = 4 / KS;                              // tiles per workgroup round
  const int kpart = wave % KS, tsub = wave / KS;
  const int ks0 = kpart, ksstep = KS;
  const bf16_t* wrow = a.Wb + (size_t)(co0 + l15) * a.Kp + 8 * lg;
  const int rounds = (a.ntiles + gridDim.x * TPW - 1) / (gridDim.x * TPW);

  // ---- per-tile state (set by setup) and the request of one k step's operands
  int n = 0, y0 = 0, x0 = 0;
  bool valid = false;
  const float* base = xin_p;
  auto setup = [&](int rnd) {
    const int pt = (rnd * gridDim.x + blockIdx.x) * TPW + tsub;
    n = pt * 16 + l15;
    valid = pt < a.ntiles && n < a.npix;
    const int nn = valid ? n : 0;
    const int b = nn / HoWo, rr = nn - b * HoWo, yo = rr / a.Wo, xo = rr - yo * a.Wo;
    y0 = yo * a.stride - pad; x0 = xo * a.stride - pad;
    base = xin_p + (size_t)b * a.H * a.W * a.Cin;
  };
  auto request = [&](int ksi) {
    StepRaw<NT> q;
    const int k = ksi * 32 + 8 * lg;
    q.c = -1;
    q.v0 = float4{0.f, 0.f, 0.f, 0.f}; q.v1 = q.v0;
    if (valid && k < K) {
      const int tap = k >> a.log2Cin, c = k & (a.Cin - 1);
      const int dy = a.ks == 3 ? (tap * 11) >> 5 : 0, dx = tap - 3 * dy;
      const int yy = y0 + dy, xx = x0 + dx;
      if (yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) {
        const float4* p = reinterpret_cast<const float4*>(base + ((size_t)yy * a.W + xx) * a.Cin + c);
        q.v0 = p[0]; q.v1 = p[1];
        q.c = c;
      }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) q.af[t] = *reinterpret_cast<const u32x4_t*>(wrow + (size_t)16 * t * a.Kp + ksi * 32);
    return q;
  };
  // The first tile's first three k steps are requested BEFORE the statistics of the input BatchNorm are folded: they do not depend on them,
  // and the fold is a round trip to the accumulator copies (+ two barriers) that every workgroup would otherwise sit out with nothing in flight.
  StepRaw<NT> q0, q1, q2;
  setup(0);
  q0 = request(ks0 < nks ? ks0 : 0); q1 = q0; q2 = q0;
  if (ks0 + ksstep < nks) q1 = request(ks0 + ksstep);
  if (ks0 + 2 * ksstep < nks) q2 = request(ks0 + 2 * ksstep);

  const bool publish = a.pub.out_mean != nullptr && blockIdx.x == 0 && blockIdx.y == 0;
  if (a.in_mode == 3 || publish) {
    // the statistics of the input BatchNorm were left as BN_COPIES partial sums by the launch that produced xin (its epilogue only adds;
    // a fold by ITS last workgroup cost 10-15 us of serial tail per launch): every workgroup folds them here, 16 independent L2 hits
    for (int o = tid; o < 2 * a.Cin; o += 256) {
      double u[BN_COPIES], t = 0.0;
#pragma unroll
      for (int q = 0; q < BN_COPIES; ++q) u[q] = in_acc_p[(size_t)q * 2 * a.Cin + o];
#pragma unroll
      for (int q = 0; q < BN_COPIES; ++q) t += u[q];
      red2c[o] = t;
    }
    __syncthreads();
    for (int c = tid; c < a.Cin; c += 256) {                // bn_apply_kernel's mean / variance / invstd
      const double m = red2c[c] / a.in_rows, v = red2c[a.Cin + c] / a.in_rows - m * m;
      const float mu = (float)m, var = (float)(v > 0.0 ? v : 0.0);
      if (a.in_mode == 3) { prm[0][c] = mu; prm[1][c] = 1.0f / sqrtf(var + a.in_eps); prm[2][c] = a.in_gamma[c]; prm[3][c] = a.in_beta[c]; }
    }
    if (publish) bn_finalize(red2c, a.Cin, a.in_rows, pub_p);
  }
  if (a.in_mode == 0 || a.in_mode == 1) {
    for (int c = tid; c < a.Cin; c += 256) {
      prm[0][c] = a.in_mean[c];
      prm[1][c] = a.in_mode == 1 ? 1.0f / sqrtf(a.in_isd[c] + a.in_eps) : a.in_isd[c];
      prm[2][c] = a.in_gamma[c];
      prm[3][c] = a.in_beta[c];
    }
  }
  __syncthreads();

  for (int rnd = 0; rnd < rounds; ++rnd) {
    if (rnd > 0) {
      setup(rnd);
      q0 = request(ks0 < nks ? ks0 : 0); q1 = q0; q2 = q0;
      if (ks0 + ksstep < nks) q1 = request(ks0 + ksstep);
      if (ks0 + 2 * ksstep < nks) q2 = request(ks0 + 2 * ksstep);
    }
    f32x4_t acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    auto consume = [&](const StepRaw<NT>& q) {
      u32x4_t bfrag = {0u, 0u, 0u, 0u};
      if (q.c >= 0) {
        float v[8] = {q.v0.x, q.v0.y, q.v0.z, q.v0.w, q.v1.x, q.v1.y, q.v1.z, q.v1.w};
        if (a.in_mode != 2) {
          const int c = q.c;
          const float4 m0 = *reinterpret_cast<const float4*>(&prm[0][c]), m1 = *reinterpret_cast<const float4*>(&prm[0][c + 4]);
          const float4 i0 = *reinterpret_cast<const float4*>(&prm[1][c]), i1 = *reinterpret_cast<const float4*>(&prm[1][c + 4]);
          const float4 g0 = *reinterpret_cast<const float4*>(&prm[2][c]), g1 = *reinterpret_cast<const float4*>(&prm[2][c + 4]);
          const float4 b0 = *reinterpret_cast<const float4*>(&prm[3][c]), b1 = *reinterpret_cast<const float4*>(&prm[3][c + 4]);
          const float mu[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w}, is[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
          const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bt[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
          for (int e = 0; e < 8; ++e) {                 // bn_apply_kernel's arithmetic, operation for operation
            const float yv = g[e] * ((v[e] - mu[e]) * is[e]) + bt[e];
            v[e] = yv > 0.f ? yv : a.slope * yv;
          }
        }
        bfrag = u32x4_t{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
      }
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, q.af[t]), __builtin_bit_cast(bf16x8_t, bfrag), acc[t], 0, 0, 0);
    };
    // three k steps requested ahead of the one being consumed: the loop waits on L2 / fabric round trips (the input was written by the
    // previous launch, mostly on other XCDs)
    for (int ksi = ks0; ksi < nks; ksi += ksstep) {
      StepRaw<NT> q3 = q2;
      if (ksi + 3 * ksstep < nks) q3 = request(ksi + 3 * ksstep);
      consume(q0);
      q0 = q1; q1 = q2; q2 = q3;
    }
    if (KS > 1) {
      if (kpart != 0) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) kred[wave][t][r][lane] = acc[t][r];
      }
      __syncthreads();
      if (kpart == 0) {
#pragma unroll
        for (int p = 1; p < KS; ++p)
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][r] += kred[wave + p][t][r][lane];
      }
    }
    // D[i][j]: i = output channel within the tile = 4 lg + r, j = pixel = l15
    if (valid && kpart == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const size_t o = (size_t)n * a.Cout + co0 + 16 * t + 4 * lg;
        f32x4_t out = acc[t];
        if (resid_p) {
          const f32x4_t rs = *reinterpret_cast<const f32x4_t*>(resid_p + o);
          out[0] += rs[0]; out[1] += rs[1]; out[2] += rs[2]; out[3] += rs[3];
        }
        *reinterpret_cast<f32x4_t*>(y_p + o) = out;
        if (stats) {
#pragma unroll
          for (int r = 0; r < 4; ++r) { s1[t][r] += out[r]; s2[t][r] += out[r] * out[r]; }
        }
      }
    }
    if (KS > 1) __syncthreads();                          // kred is free again
  }
  if (!stats) return;
  // ---- statistics: the 16 pixel lanes of a channel group -> lane l15 == 0 -> wave slot in LDS -> workgroup -> accumulator copy
  // (waves with a k part != 0 stored nothing: their sums are zero)
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float f1 = s1[t][r], f2 = s2[t][r];                    // 16 pixels x (<= 4 tiles) per channel in fp32, double from the wave slot on
      f1 = row16_sum(f1); f2 = row16_sum(f2);              // (DPP: 256 ds_bpermute round trips per wave were ~2 us of this epilogue)
      if (l15 == 0) { redw[wave][0][16 * t + 4 * lg + r] = (double)f1; redw[wave][1][16 * t + 4 * lg + r] = (double)f2; }
    }
  __syncthreads();
  double* accp = acc_out_p + (size_t)(blockIdx.x % BN_COPIES) * 2 * a.Cout;
  for (int o = tid; o < 2 * NT * 16; o += 256) {
    const int which = o / (NT * 16), ch = o % (NT * 16);
    const double tsum = redw[0][which][ch] + redw[1][which][ch] + redw[2][which][ch] + redw[3][which][ch];
    unsafeAtomicAdd(accp + which * a.Cout + co0 + ch, tsum);          // fire and forget: the next launch reads them
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// The same convolution with the INPUT TILE IN LDS (output rows of >= 16 pixels in 128 / 256-pixel blocks; 8 x 8 outputs one image per workgroup).
//
// wrn_conv_kernel above asks L2 for every operand of every k step: per 16-pixel tile and k step NT filter fragments + the pixel's 8 channels
// of one tap -- 5 loads for 4 MFMAs, the same input value fetched (and normalised) once per tap, nine times in all.  bench.py's roofline
// pass put it at 0.09 of the HBM roof (70 TFLOP/s) whether a launch carried one pass or nine: not launch overhead, the operand path.
// Here a workgroup owns a TH x TW block of output pixels (128 or 256) of one image:
//   * the (TH s + k - s) x (TW s + k - s) input block is read ONCE, normalised + activated ONCE with bn_apply_kernel's arithmetic, rounded to
//     bf16 and kept in LDS ([pixel][Cin + 8]: the 16-byte pad makes the pixel pitch an odd number of 16-byte bank groups); out-of-image
//     pixels are the zeros of the convolution's padding;
//   * B fragments (8 channels of one tap of one pixel) are ds_read_b128s; a filter fragment from L2 (three k steps ahead) feeds PG MFMAs
//     -- the PG 16-pixel groups a wave owns -- instead of one;
//   * k order, accumulation order and the epilogue (residual, store, statistics of the output into the next BatchNorm's accumulator
//     copies) are wrn_conv_kernel's, so the two kernels agree to the last bit on the layers both can run.
template <int NT, int PG>
__global__ __launch_bounds__(256, 2) void wrn_conv_tile_kernel(const ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) bf16_t tin[];          // [IH * IW][Cin + 8]
  __shared__ float prm[4][128];
  __shared__ double redw[4][2][NT * 16];
  __shared__ double red2c[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int co0 = blockIdx.y * NT * 16, K = a.ks * a.ks * a.Cin, pad = a.ks >> 1, nks = a.Kp >> 5;
  const bool stats = a.acc_out != nullptr;
  const int ps = blockIdx.z;
  const float* const xin_p = a.xin + (size_t)ps * a.in_ps;
  float* const y_p = a.y + (size_t)ps * a.out_ps;
  const float* const resid_p = a.resid ? a.resid + (size_t)ps * a.out_ps : nullptr;
  const double* const in_acc_p = a.in_acc ? a.in_acc + (size_t)ps * BN_COPIES * 2 * a.Cin : nullptr;
  double* const acc_out_p = a.acc_out ? a.acc_out + (size_t)ps * BN_COPIES * 2 * a.Cout : nullptr;
  BnFinal pub_p = a.pub;
  if (pub_p.out_mean) { pub_p.out_mean += (size_t)ps * a.Cin; pub_p.out_invstd += (size_t)ps * a.Cin; }
  pub_p.update_running = a.pub.update_running && ps == 0;
  // block -> (image, tile row, tile column)
  const int tpi = a.tiles_x * a.tiles_y;
  const int bq = blockIdx.x / tpi, tr = (blockIdx.x - bq * tpi) / a.tiles_x, tc = blockIdx.x - bq * tpi - tr * a.tiles_x;
  const int b = bq * a.ipw;                                              // first image of the workgroup
  const int blk_px = a.TH * a.TW, blk_in = a.IH * a.IW;
  const int oy0 = tr * a.TH, ox0 = tc * a.TW;
  const int iy0 = oy0 * a.stride - pad, ix0 = ox0 * a.stride - pad;
  const int PP = a.Cin + 8;                                             // LDS pixel pitch (elements)

  // filter fragments of the first three k steps: requested before anything else (they depend on nothing)
  const bf16_t* wrow = a.Wb + (size_t)(co0 + l15) * a.Kp + 8 * lg;
  struct WF { u32x4_t af[NT]; };
  auto wreq = [&](int ksi) {
    WF q;
#pragma unroll
    for (int t = 0; t < NT; ++t) q.af[t] = *reinterpret_cast<const u32x4_t*>(wrow + (size_t)16 * t * a.Kp + ksi * 32);
    return q;
  };
  WF w0 = wreq(0), w1 = w0, w2 = w0;
  if (1 < nks) w1 = wreq(1);
  if (2 < nks) w2 = wreq(2);

  const bool publish = a.pub.out_mean != nullptr && blockIdx.x == 0 && blockIdx.y == 0;
  if (a.in_mode == 3 || publish) {
    for (int o = tid; o < 2 * a.Cin; o += 256) {
      double u[BN_COPIES], t = 0.0;
#pragma unroll
      for (int q = 0; q < BN_COPIES; ++q) u[q] = in_acc_p[(size_t)q * 2 * a.Cin + o];
#pragma unroll
      for (int q = 0; q < BN_COPIES; ++q) t += u[q];
      red2c[o] = t;
    }
    __syncthreads();
    for (int c = tid; c < a.Cin; c += 256) {                // bn_apply_kernel's mean / variance / invstd
      const double m = red2c[c] / a.in_rows, v = red2c[a.Cin + c] / a.in_rows - m * m;
      const float mu = (float)m, var = (float)(v > 0.0 ? v : 0.0);
      if (a.in_mode == 3) { prm[0][c] = mu; prm[1][c] = 1.0f / sqrtf(var + a.in_eps); prm[2][c] = a.in_gamma[c]; prm[3][c] = a.in_beta[c]; }
    }
    if (publish) bn_finalize(red2c, a.Cin, a.in_rows, pub_p);
  }
  if (a.in_mode == 0 || a.in_mode == 1) {
    for (int c = tid; c < a.Cin; c += 256) {
      prm[0][c] = a.in_mean[c];
      prm[1][c] = a.in_mode == 1 ? 1.0f / sqrtf(a.in_isd[c] + a.in_eps) : a.in_isd[c];
      prm[2][c] = a.in_gamma[c];
      prm[3][c] = a.in_beta[c];
    }
  }
  __syncthreads();

  // ---- the input block: fp32 NHWC -> BatchNorm + LeakyReLU -> bf16 -> LDS (4 channels per thread and step)
  {
    const int c4n = a.Cin >> 2, total = a.ipw * blk_in * c4n;
    const float* img0 = xin_p + (size_t)b * a.H * a.W * a.Cin;
    for (int e0 = tid; e0 < total; e0 += 4 * 256) {
      float4 v[4];
      int pix[4], cc[4];
      bool in[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {                          // four requests in flight per thread
        const int e = e0 + u * 256;
        pix[u] = e / c4n; cc[u] = (e - pix[u] * c4n) << 2;
        const int il = pix[u] / blk_in, pr = pix[u] - il * blk_in;
        const int iy = pr / a.IW, ix = pr - iy * a.IW, yy = iy0 + iy, xx = ix0 + ix;
        in[u] = e < total && yy >= 0 && yy < a.H && xx >= 0 && xx < a.W;
        v[u] = float4{0.f, 0.f, 0.f, 0.f};
        if (in[u]) v[u] = *reinterpret_cast<const float4*>(img0 + ((size_t)(il * a.H + yy) * a.W + xx) * a.Cin + cc[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (e0 + u * 256 >= total) break;
        float o[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        if (in[u] && a.in_mode != 2) {
          const int c = cc[u];
          const float4 m0 = *reinterpret_cast<const float4*>(&prm[0][c]), i0 = *reinterpret_cast<const float4*>(&prm[1][c]);
          const float4 g0 = *reinterpret_cast<const float4*>(&prm[2][c]), b0 = *reinterpret_cast<const float4*>(&prm[3][c]);
          const float mu[4] = {m0.x, m0.y, m0.z, m0.w}, is[4] = {i0.x, i0.y, i0.z, i0.w};
          const float g[4] = {g0.x, g0.y, g0.z, g0.w}, bt[4] = {b0.x, b0.y, b0.z, b0.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {                      // bn_apply_kernel's arithmetic, operation for operation
            const float yv = g[q] * ((o[q] - mu[q]) * is[q]) + bt[q];
            o[q] = yv > 0.f ? yv : a.slope * yv;
          }
        }
        const u32x2_t pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};      // (padding pixels: zeros)
        *reinterpret_cast<u32x2_t*>(tin + (size_t)pix[u] * PP + cc[u]) = pk;
      }
    }
  }
  __syncthreads();

  // ---- main loop: the wave's PG pixel groups x NT channel tiles
  int pb[PG];                                               // LDS element offset of the pixel's tap (0, 0)
  int n_out[PG];
#pragma unroll
  for (int gi = 0; gi < PG; ++gi) {
    const int p = (wave * PG + gi) * 16 + l15, il = p / blk_px, q = p - il * blk_px, ty = q / a.TW, tx = q - ty * a.TW;
    pb[gi] = (il * blk_in + (ty * a.stride) * a.IW + tx * a.stride) * PP;
    n_out[gi] = ((b + il) * a.Ho + oy0 + ty) * a.Wo + ox0 + tx;
  }
  f32x4_t acc[PG][NT];
#pragma unroll
  for (int gi = 0; gi < PG; ++gi)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[gi][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int ksi = 0; ksi < nks; ++ksi) {
    WF w3 = w2;
    if (ksi + 3 < nks) w3 = wreq(ksi + 3);
    const int k = ksi * 32 + 8 * lg;
    int toff = -1;
    if (k < K) {
      const int tap = k >> a.log2Cin, c = k & (a.Cin - 1);
      const int dy = a.ks == 3 ? (tap * 11) >> 5 : 0, dx = tap - 3 * dy;
      toff = (dy * a.IW + dx) * PP + c;
    }
#pragma unroll
    for (int gi = 0; gi < PG; ++gi) {
      u32x4_t bfrag = {0u, 0u, 0u, 0u};
      if (toff >= 0) bfrag = *reinterpret_cast<const u32x4_t*>(tin + pb[gi] + toff);
#pragma unroll
      for (int t = 0; t < NT; ++t)
        acc[gi][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, w0.af[t]), __builtin_bit_cast(bf16x8_t, bfrag),
                                                             acc[gi][t], 0, 0, 0);
    }
    w0 = w1; w1 = w2; w2 = w3;
  }
  // ---- epilogue: D[i][j]: i = output channel within the tile = 4 lg + r, j = pixel = l15
  float s1[NT][4], s2[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[t][r] = 0.f; s2[t][r] = 0.f; }
#pragma unroll
  for (int gi = 0; gi < PG; ++gi) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const size_t o = (size_t)n_out[gi] * a.Cout + co0 + 16 * t + 4 * lg;
      f32x4_t out = acc[gi][t];
      if (resid_p) {
        const f32x4_t rs = *reinterpret_cast<const f32x4_t*>(resid_p + o);
        out[0] += rs[0]; out[1] += rs[1]; out[2] += rs[2]; out[3] += rs[3];
      }
      *reinterpret_cast<f32x4_t*>(y_p + o) = out;
      if (stats) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { s1[t][r] += out[r]; s2[t][r] += out[r] * out[r]; }
      }
    }
  }
  if (!stats) return;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float f1 = row16_sum(s1[t][r]), f2 = row16_sum(s2[t][r]);
      if (l15 == 0) { redw[wave][0][16 * t + 4 * lg + r] = (double)f1; redw[wave][1][16 * t + 4 * lg + r] = (double)f2; }
    }
  __syncthreads();
  double* accp = acc_out_p + (size_t)(blockIdx.x % BN_COPIES) * 2 * a.Cout;
  for (int o = tid; o < 2 * NT * 16; o += 256) {
    const int which = o / (NT * 16), ch = o % (NT * 16);
    const double tsum = redw[0][which][ch] + redw[1][which][ch] + redw[2][which][ch] + redw[3][which][ch];
    unsafeAtomicAdd(accp + which * a.Cout + co0 + ch, tsum);
  }
}

__global__ __launch_bounds__(256) void bn_act_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ isd,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float slope,
                                                    int mode, bf16_t* __restrict__ act, float* __restrict__ act_f32, size_t n4, int C) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // over rows * C / 4
  if (i >= n4) return;
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  float o[4] = {v.x, v.y, v.z, v.w};
  if (mode != 2) {
    const int c = (int)((i * 4) % C);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float is = mode == 1 ? 1.0f / sqrtf(isd[c + e] + eps) : isd[c + e];
      const float yv = gamma[c + e] * ((o[e] - mean[c + e]) * is) + beta[c + e];
      o[e] = yv > 0.f ? yv : slope * yv;
    }
  }
  if (act) {
    u32x2_t pk = {pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
    reinterpret_cast<u32x2_t*>(act)[i] = pk;
  }
  if (act_f32) reinterpret_cast<float4*>(act_f32)[i] = float4{o[0], o[1], o[2], o[3]};
}

// The network's tail in one launch per image batch (wrn.py:119-126): final BatchNorm + LeakyReLU (statistics folded from the accumulator the
// last convolution filled, or the running statistics), global average pooling, classifier.  One workgroup per image; workgroup 0 publishes the
// BatchNorm's mean / invstd / running statistics.  (Four launches before: fold, apply, pool, classifier -- 32 us per forward.)
struct HeadArgs {
  const float* x; const float* in_mean; const float* in_isd; const double* in_acc; const float* gamma; const float* beta;
  float eps, slope; int in_mode; BnFinal pub;
  const float* Wc; const float* bc; float* feat; float* logits;
  int HW2, C, K, in_rows;
  int Bp;                      // images per pass (blockIdx.x / Bp = the pass: its own accumulator, its own published statistics)
};
__global__ __launch_bounds__(256) void wrn_head_kernel(const HeadArgs a) {
  __shared__ double red2c[512];
  __shared__ float prm[4][256];
  __shared__ float part[256];
  __shared__ float ft[256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, C = a.C;
  const int ps = b / a.Bp;
  if (a.in_mode == 3) {
    const double* in_acc_p = a.in_acc + (size_t)ps * BN_COPIES * 2 * C;
    for (int o = tid; o < 2 * C; o += 256) {
      double u[BN_COPIES], t = 0.0;
#pragma unroll
      for (int q = 0; q < BN_COPIES; ++q) u[q] = in_acc_p[(size_t)q * 2 * C + o];
#pragma unroll
      for (int q = 0; q < BN_COPIES; ++q) t += u[q];
      red2c[o] = t;
    }
    __syncthreads();
    for (int c = tid; c < C; c += 256) {
      const double m = red2c[c] / a.in_rows, v = red2c[C + c] / a.in_rows - m * m;
      prm[0][c] = (float)m; prm[1][c] = 1.0f / sqrtf((float)(v > 0.0 ? v : 0.0) + a.eps); prm[2][c] = a.gamma[c]; prm[3][c] = a.beta[c];
    }
    if (b % a.Bp == 0) {
      BnFinal pub_p = a.pub;
      if (pub_p.out_mean) { pub_p.out_mean += (size_t)ps * C; pub_p.out_invstd += (size_t)ps * C; }
      pub_p.update_running = a.pub.update_running && ps == 0;
      bn_finalize(red2c, C, a.in_rows, pub_p);
    }
  } else {
    for (int c = tid; c < C; c += 256) {
      prm[0][c] = a.in_mean[c];
      prm[1][c] = a.in_mode == 1 ? 1.0f / sqrtf(a.in_isd[c] + a.eps) : a.in_isd[c];
      prm[2][c] = a.gamma[c]; prm[3][c] = a.beta[c];
    }
  }
  __syncthreads();
  // pooled features: thread = (pixel group, channel); the groups' partial sums meet in LDS in group order
  const int groups = 256 / C > 0 ? 256 / C : 1;
  for (int c0 = 0; c0 < C; c0 += 256) {
    const int c = c0 + tid % (groups > 1 ? C : 256), grp = groups > 1 ? tid / C : 0;
    float s = 0.f;
    if (c < C && grp < groups) {
      const float mu = prm[0][c], is = prm[1][c], g = prm[2][c], bt = prm[3][c];
      const float* xb = a.x + (size_t)b * a.HW2 * C + c;
      int p = grp;
      for (; p + 7 * groups < a.HW2; p += 8 * groups) {        // 8 loads in flight (a dependent chain of 32 round trips otherwise)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = xb[(size_t)(p + u * groups) * C];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const float yv = g * ((v[u] - mu) * is) + bt;                                     // bn_apply_kernel's arithmetic
          s += yv > 0.f ? yv : a.slope * yv;
        }
      }
      for (; p < a.HW2; p += groups) {
        const float yv = g * ((xb[(size_t)p * C] - mu) * is) + bt;
        s += yv > 0.f ? yv : a.slope * yv;
      }
    }
    part[tid] = s;
    __syncthreads();
    if (grp == 0 && c < C) {
      float t = 0.f;
      for (int q = 0; q < groups; ++q) t += part[q * C + (groups > 1 ? c : tid)];
      t /= a.HW2;
      ft[c] = t;
      a.feat[(size_t)b * C + c] = t;
    }
    __syncthreads();
  }
  // classifier: one wave per output, lanes along the features (fc_fwd_kernel's order of the sums); the filter rows of 8 outputs are requested
  // before the first is used (a dependent L2 round trip per output otherwise: 25 of them per wave)
  const int nf = (C + 63) / 64;                     // features per lane (<= 4)
  for (int k0 = wave; k0 < a.K; k0 += 32) {
    float w[8][4];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = k0 + 4 * u, f = lane + 64 * q;
        w[u][q] = (k < a.K && q < nf && f < C) ? a.Wc[(size_t)k * C + f] : 0.f;
      }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + 4 * u;
      if (k >= a.K) break;
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) if (q < nf) s += ft[(lane + 64 * q) < C ? lane + 64 * q : 0] * w[u][q];
      s = rows_sum4(row16_sum(s));                 // DPP + row swaps instead of six ds_bpermute round trips
      if (lane == 0) a.logits[(size_t)b * a.K + k] = s + a.bc[k];
    }
  }
}

}  // namespace

extern "C" int srhip_wrn_head(const float* x, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc, const float* gamma,
                              const float* beta, float eps, float slope, float* pub_mean, float* pub_invstd, float* running_mean,
                              float* running_var, float momentum, int update_running, const float* Wc, const float* bc, float* feat,
                              float* logits, int B, int HW2, int C, int K, int stat_ranks, void* stream) {
  return srhip_wrn_head_passes(x, in_mode, in_mean, in_isd, in_acc, gamma, beta, eps, slope, pub_mean, pub_invstd, running_mean, running_var, momentum,
                               update_running, Wc, bc, feat, logits, B, HW2, C, K, stat_ranks, 1, stream);
}

extern "C" int srhip_wrn_head_passes(const float* x, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc, const float* gamma,
                                     const float* beta, float eps, float slope, float* pub_mean, float* pub_invstd, float* running_mean,
                                     float* running_var, float momentum, int update_running, const float* Wc, const float* bc, float* feat,
                                     float* logits, int B, int HW2, int C, int K, int stat_ranks, int passes, void* stream) {
  if (!x || !gamma || !beta || !Wc || !bc || !feat || !logits || B <= 0 || HW2 <= 0 || C <= 0 || C > 256 || K <= 0 || passes <= 0) return SR_EINVAL;
  if (passes > 1 && in_mode != 3) return SR_EINVAL;                // passes = statistics groups: batch statistics only
  if (in_mode != 0 && in_mode != 1 && in_mode != 3) return SR_EINVAL;
  if (in_mode == 3 ? !in_acc : (!in_mean || !in_isd)) return SR_EINVAL;
  if (pub_mean && (in_mode != 3 || !pub_invstd || (update_running && (!running_mean || !running_var)))) return SR_EINVAL;
  HeadArgs a;
  a.x = x; a.in_mean = in_mean; a.in_isd = in_isd; a.in_acc = in_acc; a.gamma = gamma; a.beta = beta; a.eps = eps; a.slope = slope;
  a.in_mode = in_mode;
  a.pub.out_mean = pub_mean; a.pub.out_invstd = pub_invstd; a.pub.running_mean = running_mean; a.pub.running_var = running_var;
  a.pub.momentum = momentum; a.pub.update_running = update_running; a.pub.eps = eps;
  a.Wc = Wc; a.bc = bc; a.feat = feat; a.logits = logits; a.HW2 = HW2; a.C = C; a.K = K;
  a.in_rows = B * HW2 * (stat_ranks > 1 ? stat_ranks : 1);
  a.Bp = B;
  SR_LAUNCH(wrn_head_kernel, dim3(B * passes), dim3(256), 0, (hipStream_t)stream, a);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_wrn_conv_supported(int Cin, int Cout, int ksize) {
  return (ksize == 1 || ksize == 3) && Cin >= 8 && Cin <= 128 && (Cin & (Cin - 1)) == 0 && Cout <= 256 &&
         (Cout == 16 || Cout == 32 || (Cout >= 64 && Cout % 64 == 0));
}

extern "C" long long srhip_bn_acc_doubles(int C) { return (long long)BN_COPIES * 2 * C; }

extern "C" int srhip_wrn_conv_bn(const float* xin, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc,
                                 const float* in_gamma, const float* in_beta, float in_eps, float slope, float* pub_mean, float* pub_invstd,
                                 float* running_mean, float* running_var, float momentum, int update_running, const void* Wb,
                                 const float* resid, float* y, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int Kpad,
                                 double* acc_out, int stat_ranks, void* stream) {
  return srhip_wrn_conv_bn_passes(xin, in_mode, in_mean, in_isd, in_acc, in_gamma, in_beta, in_eps, slope, pub_mean, pub_invstd, running_mean,
                                  running_var, momentum, update_running, Wb, resid, y, B, H, W, Cin, Cout, ksize, stride, Kpad, acc_out, stat_ranks, 1,
                                  stream);
}

// Which template the dispatcher below launched last (diagnostic: bench.py names the kernel of its roofline object after the launch it timed):
// tile kernel 100 + 10 NT + PG, direct kernel 10 NT + KS.
static int g_last_conv_plan = 0;
extern "C" int srhip_wrn_conv_last_plan() { return g_last_conv_plan; }

namespace {

// The launcher's host decisions -- the ONE spelling of them: srhip_wrn_conv_bn_passes launches what conv_plan says, srhip_wrn_conv_plan reports it.
struct ConvPlan {
  int kernel;                  // 100 + 10 NT + PG (wrn_conv_tile_kernel) | 10 NT + KS (wrn_conv_kernel)
  int NT, gy, PG, KS;          // PG: tile kernel only; KS: direct kernel only (0 otherwise)
  int grid_x, rounds;          // rounds: the direct kernel's grid-stride loop count (1 for the tile kernel)
  int Ho, Wo, npix, ntiles;
  int TW, TH, IW, IH, tiles_x, tiles_y, ipw;
  size_t smem;
};

// Kpad < 0: K = Cin k k rounded up to 32, as the callers of conv_weight_prep pad it
int conv_plan(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int Kpad, int passes, ConvPlan& p) {
  if (B <= 0 || H <= 0 || W <= 0 || stride <= 0 || !srhip_wrn_conv_supported(Cin, Cout, ksize) || passes <= 0 || passes > 64) return SR_EINVAL;
  if (Kpad < 0) Kpad = (Cin * ksize * ksize + 31) / 32 * 32;
  if (Kpad < Cin * ksize * ksize || (Kpad % 32)) return SR_EINVAL;
  const int pad = ksize >> 1;
  p.Ho = (H + 2 * pad - ksize) / stride + 1; p.Wo = (W + 2 * pad - ksize) / stride + 1;
  p.npix = B * p.Ho * p.Wo; p.ntiles = cdiv(p.npix, 16);
  const int NT = Cout >= 64 ? 4 : Cout / 16;                       // 16 -> 1, 32 -> 2, >= 64 -> 4
  const int gy = Cout / (NT * 16), nks = Kpad / 32;
  p.NT = NT; p.gy = gy; p.PG = 0; p.KS = 0; p.rounds = 1;
  p.TW = p.TH = p.IW = p.IH = p.tiles_x = p.tiles_y = 0; p.ipw = 1; p.smem = 0;
  // layers with >= 16 output pixels per row and whole 128 / 256-pixel blocks: the input block in LDS (wrn_conv_tile_kernel)
  static const bool no_tile = SR_TUNE_ENV("SRHIP_CONV_NO_TILE") != nullptr;
  if (!no_tile && ((p.Wo >= 16 && (p.Wo % 16) == 0) || (p.Wo == 8 && p.Ho == 8)) && NT >= 2 && Cin % 4 == 0) {
    const int TW = (p.Wo % 32) == 0 ? 32 : (p.Wo == 8 ? 8 : 16);
    // 128 pixels per workgroup (PG = 2); 256 (PG = 4: every filter fragment feeds four MFMAs) when the launch still has >= 4 workgroups per
    // CU and the input block stays within 64 KB (two workgroups per CU)
    auto geom = [&](int PG_) {
      p.ipw = p.Wo == 8 ? PG_ : 1;
      p.TW = TW; p.TH = 64 * PG_ / (TW * p.ipw); p.IW = (TW - 1) * stride + ksize; p.IH = (p.TH - 1) * stride + ksize;
      p.tiles_x = p.Wo / TW; p.tiles_y = p.Ho / p.TH;
      return (size_t)p.ipw * p.IH * p.IW * (Cin + 8) * sizeof(bf16_t);
    };
    int PG = 4;
    size_t smem = geom(4);
    if ((long)B * passes * p.Ho * p.Wo / 256 * gy < 1024 || p.Ho % p.TH != 0 || smem > 64 * 1024) { PG = 2; smem = geom(2); }
    if (p.Wo == 8) {                                                 // the 8 x 8 stage: whole images, two per workgroup when the batch is even
      PG = (B % 2 == 0) ? 2 : 1;
      smem = geom(PG);
      if (smem > 64 * 1024 && PG == 2) { PG = 1; smem = geom(1); }   // (the stride-2 layer into this stage: 17 x 17 input pixels per image)
    }
    if (p.Ho % p.TH == 0 && smem <= 64 * 1024) {
      p.PG = PG; p.smem = smem;
      p.grid_x = B / p.ipw * p.tiles_x * p.tiles_y;
      p.kernel = 100 + 10 * (NT == 4 ? 4 : 2) + PG;
      return SR_OK;
    }
  }
  // <= 512 workgroups (tools/wrn_conv_bench.py: 1024 cost +2.6 us with the statistics prologue / epilogue per workgroup); the waves of a
  // workgroup split K (2 or 4 ways) until the launch has ~2048 waves, as long as a wave keeps >= 4 k steps
  static const int env_ks = SR_TUNE_ENV("SRHIP_CONV_KSPLIT") ? atoi(SR_TUNE_ENV("SRHIP_CONV_KSPLIT")) : 0;          // tuning: force 1 / 2 / 4
  static const int env_maxwg = SR_TUNE_ENV("SRHIP_CONV_MAXWG") ? atoi(SR_TUNE_ENV("SRHIP_CONV_MAXWG")) : 512;
  int KS = 1;
  while (KS < 4 && (long)p.ntiles * passes * gy * KS * 2 <= 2048 && nks / (KS * 2) >= 4) KS *= 2;
  if (env_ks == 1 || env_ks == 2 || env_ks == 4) KS = env_ks;
  // workgroups per pass: the launch as a whole stays at <= env_maxwg workgroups (two rounds of the chip) however many passes share it --
  // every workgroup pays the statistics prologue / epilogue once and then walks more pixel tiles
  int gx = cdiv(p.ntiles, 4 / KS);
  const int cap = env_maxwg * (passes > 1 ? 2 : 1) / (gy * passes);
  if (gx > cap) gx = cap;
  if (gx < 1) gx = 1;
  p.KS = KS; p.grid_x = gx;
  p.rounds = cdiv(p.ntiles, gx * (4 / KS));                        // wrn_conv_kernel's `rounds`
  p.kernel = 10 * NT + KS;
  return SR_OK;
}

}  // namespace

extern "C" int srhip_wrn_conv_plan(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int passes, int* kernel, int* grid_x, int* rounds) {
  ConvPlan p;
  const int rc = conv_plan(B, H, W, Cin, Cout, ksize, stride, -1, passes, p);
  if (rc != SR_OK) return rc;
  if (kernel) *kernel = p.kernel;
  if (grid_x) *grid_x = p.grid_x;
  if (rounds) *rounds = p.rounds;
  return SR_OK;
}

extern "C" int srhip_wrn_conv_bn_passes(const float* xin, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc,
                                        const float* in_gamma, const float* in_beta, float in_eps, float slope, float* pub_mean, float* pub_invstd,
                                        float* running_mean, float* running_var, float momentum, int update_running, const void* Wb,
                                        const float* resid, float* y, int B, int H, int W, int Cin, int Cout, int ksize, int stride, int Kpad,
                                        double* acc_out, int stat_ranks, int passes, void* stream) {
  ConvPlan p;
  if (!xin || !Wb || !y || in_mode < 0 || in_mode > 3 || Kpad < 0 || conv_plan(B, H, W, Cin, Cout, ksize, stride, Kpad, passes, p) != SR_OK) return SR_EINVAL;
  if (passes > 1 && (in_mode == 0 || in_mode == 1)) return SR_EINVAL;     // statistics handed in are one group's: passes fold their own (3) or read raw (2)
  if ((in_mode == 0 || in_mode == 1) && (!in_mean || !in_isd)) return SR_EINVAL;
  if (in_mode != 2 && (!in_gamma || !in_beta)) return SR_EINVAL;
  if ((in_mode == 3 || pub_mean) && !in_acc) return SR_EINVAL;
  if (pub_mean && (!pub_invstd || (update_running && (!running_mean || !running_var)))) return SR_EINVAL;
  ConvArgs a;
  a.xin = xin; a.in_mean = in_mean; a.in_isd = in_isd; a.in_gamma = in_gamma; a.in_beta = in_beta; a.in_acc = in_acc;
  a.in_eps = in_eps; a.slope = slope; a.in_mode = in_mode;
  a.pub.out_mean = pub_mean; a.pub.out_invstd = pub_invstd; a.pub.running_mean = running_mean; a.pub.running_var = running_var;
  a.pub.momentum = momentum; a.pub.update_running = update_running; a.pub.eps = in_eps;
  a.Wb = (const bf16_t*)Wb; a.resid = resid; a.y = y;
  a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.ks = ksize; a.stride = stride; a.Kp = Kpad;
  a.in_rows = B * H * W * (stat_ranks > 1 ? stat_ranks : 1);       // SyncBatchNorm: the accumulator holds every rank's sums
  a.log2Cin = 0;
  while ((1 << a.log2Cin) < Cin) ++a.log2Cin;
  a.Ho = p.Ho; a.Wo = p.Wo; a.npix = p.npix; a.ntiles = p.ntiles;
  a.acc_out = acc_out;
  a.in_ps = (long)B * H * W * Cin; a.out_ps = (long)a.npix * Cout;
  a.TW = p.TW; a.TH = p.TH; a.IW = p.IW; a.IH = p.IH; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.ipw = p.ipw;
  hipStream_t s = (hipStream_t)stream;
  if (p.kernel >= 100) {
    const size_t smem = p.smem;
    const dim3 grid(p.grid_x, p.gy, passes);
#define SR_TILE_LAUNCH(NT_, PG_)                                                                                           \
    do {                                                                                                                  \
      auto kern = wrn_conv_tile_kernel<NT_, PG_>;                                                                         \
      if (smem > 48 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem); \
      SR_LAUNCH(kern, grid, dim3(256), smem, s, a);                                                                       \
    } while (0)
    switch (p.kernel) {
      case 141: SR_TILE_LAUNCH(4, 1); break;
      case 121: SR_TILE_LAUNCH(2, 1); break;
      case 144: SR_TILE_LAUNCH(4, 4); break;
      case 142: SR_TILE_LAUNCH(4, 2); break;
      case 124: SR_TILE_LAUNCH(2, 4); break;
      case 122: SR_TILE_LAUNCH(2, 2); break;
      default: return SR_EINVAL;
    }
#undef SR_TILE_LAUNCH
    g_last_conv_plan = p.kernel;
    SR_CHECK_LAUNCH();
    return SR_OK;
  }
  const int KS = p.KS;
  const dim3 grid(p.grid_x, p.gy, passes);
#define SR_CONV_LAUNCH(NT_)                                                                                          \
  if (KS == 4) SR_LAUNCH((wrn_conv_kernel<NT_, 4>), grid, dim3(256), 0, s, a);                                      \
  else if (KS == 2) SR_LAUNCH((wrn_conv_kernel<NT_, 2>), grid, dim3(256), 0, s, a);                                 \
  else SR_LAUNCH((wrn_conv_kernel<NT_, 1>), grid, dim3(256), 0, s, a)
  if (p.NT == 4) { SR_CONV_LAUNCH(4); }
  else if (p.NT == 2) { SR_CONV_LAUNCH(2); }
  else if (p.NT == 1) { SR_CONV_LAUNCH(1); }
  else return SR_EINVAL;
#undef SR_CONV_LAUNCH
  g_last_conv_plan = p.kernel;
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_bn_act(const float* x, const float* mean, const float* invstd_or_var, const float* gamma, const float* beta, float eps,
                            float slope, int mode, void* act_bf16, float* act_f32, int rows, int C, void* stream) {
  if (!x || (!act_bf16 && !act_f32) || rows <= 0 || C <= 0 || (C % 4) || mode < 0 || mode > 2) return SR_EINVAL;
  if (mode != 2 && (!mean || !invstd_or_var || !gamma || !beta)) return SR_EINVAL;
  const size_t n4 = (size_t)rows * C / 4;
  SR_LAUNCH(bn_act_kernel, dim3(cdiv(n4, 256)), dim3(256), 0, (hipStream_t)stream, x, mean, invstd_or_var, gamma, beta, eps, slope, mode,
                     (bf16_t*)act_bf16, act_f32, n4, C);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
