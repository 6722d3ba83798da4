// Fused inference MLP half of a transformer block (gfx950):
//     x <- x + row_scale * ( fc2( GELU( fc1( LayerNorm(x) ) ) ) + b2 )            reference: semilearn/nets/vit/vit.py:165
// (Block.forward, second residual: x + drop_path2(ls2(mlp(norm2(x))))), Mlp.forward vit.py:69-75.
//
// Why: at the reference batch 200 of the 216 images of a step are forwarded WITHOUT a backward (the K weak/strong passes that
// only feed the rewarder / the masks).  As three launches (LN, fc1+GELU, fc2+residual) the [M, 4D] hidden activation makes a
// round trip through HBM (2 x 158 MB per layer at M = 51400) and LN re-reads x; fused, HBM sees x in, x out.
//
// Structure (one workgroup = 128 rows, 8 waves x 16 rows, ONE workgroup per CU, 254 VGPRs):
//   * every wave owns 16 rows end to end: it normalises them in registers (bf16 MFMA B-fragments, 48 VGPRs), so neither x
//     nor the hidden activation ever sits in LDS -- all 128 KiB of the ring hold WEIGHT tiles.
//   * weights stream through a 16-slot LDS-DMA ring of 8 KiB tiles ([128 rows x 32 k] bf16, buffer_load ... lds); per
//     64-wide hidden chunk c, 12 stages of 8 MFMAs per wave:
//       stages 0-5  (GEMM1): W1 rows of hidden pair-group u = j/3 (32 hidden) x k-steps 4(j%3) .. +3
//       stages 6-11 (GEMM2): W2 rows 128 th .. (th = j%3) x hidden 64 c + 32 u .., u = (j-6)/3
//     so the accumulators of group u = 0 are complete after stage 2 and its GELU (VALU) has stages 3-5 to hide under; u = 1
//     is finished by stage 5 and needed by stage 9.
//   * GEMM1: D1 = mfma(W1 frag, xn frag): lane (m = lane&15, g = lane>>4) receives rows 4g..4g+3 of the A tile.  A-tile row i
//     of tile P is fed with hidden unit 8 (i>>2) + (i&3), tile Q with 8 (i>>2) + 4 + (i&3) (just the LDS row each lane
//     reads), so after GELU + bias + bf16 pack the lane holds hidden 8g .. 8g+7 of the group: exactly the B fragment of
//     k-step u of GEMM2 -- the chained-MFMA trick, the hidden activation never leaves registers.
//   * software pipeline inside every wave (fragments of stage s+1 requested before the MFMAs of stage s, two fragment sets),
//     one barrier per GS stages, no branches in the loop body (out-of-range ring refills are buffer-OOB no-ops that keep the
//     vmcnt arithmetic uniform).
//   * epilogue: re-read x (fp32), add, store.
// Measured alternatives (tools/microbench.py mlp, M = 51400): 4 waves x 32 rows (one wave per SIMD, every fragment feeding
// two MFMAs, 512 registers) 357 us vs 248 us for this layout -- a lone wave per SIMD stalls at every s_waitcnt; lockstep
// stages without the in-wave prefetch 330 us; GELU in one lump per chunk +10 us.  PMC of this kernel: MFMA pipe 19 % busy, LDS
// array 21 %, VALU 18 %, waves 30 % of their time in s_waitcnt: latency-, not throughput-bound at two waves per SIMD.
// Rounding points are the ones of the unfused path (xn bf16, GELU output bf16, fp32 accumulation), so the two paths agree to
// fp32 summation order.
#include <stdlib.h>

#include <utility>

#include "../../include/srhip.h"
#include "common.h"

namespace {

constexpr int BK = 32;
constexpr int RT = 128;                   // rows (weights) per ring tile
constexpr int TILE_EL = RT * BK;          // 4096 bf16 = 8 KiB
constexpr int NS = 16;                    // ring slots
constexpr int FBM = 128;                  // x rows per workgroup
constexpr int CH = 64;                    // hidden units per chunk (acc1 = 4 tiles: 16 VGPRs; 128 would not fit 256 VGPRs)

__device__ __forceinline__ int swz(int row) { return (0x78 >> (((row >> 2) & 3) * 2)) & 3; }   // as in gemm.hip

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;
template <int N_>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory"); }

// compile-time loop: f(std::integral_constant<int, 0>{}), ..., f(<N-1>) -- the stage index must be a constant expression
// (s_waitcnt immediates, accumulator indices)
template <class F, int... Is>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) { (f(std::integral_constant<int, Is>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

struct MlpArgs {
  const float* x;          // input residual stream (LayerNorm source and residual term)
  float* xo;               // output residual stream (== x for the in-place call)
  // activations kept for the backward of the first ``save_rows`` rows (the gradient-carrying images of a mixed batch), or NULL
  bf16_t *s_ln2, *s_pre, *s_h;     // [save_rows, D], [save_rows, Hd], [save_rows, Hd]
  float *s_mean, *s_rstd;          // [save_rows]
  int save_rows;
  const float *gamma, *beta, *b1, *b2, *row_scale;
  const bf16_t *W1, *W2;
  // PROJ variant (rows without a backward): the attention output projection + first residual of the block run in this launch too,
  //   x <- x + row_scale1 * (ao Wp^T + bp)      (vit.py:163 after Attention.forward :105-106), then the MLP half on the result
  const bf16_t *ao, *Wp;   // [M, D] attention output (heads concatenated), [D, D]
  const float *bp, *row_scale1;
  int ao_scaled;           // the producer of ao (srhip_attn_block_fused out_scale) already applied row_scale1 to it
  // PROJ variant, optional: LayerNorm of the OUTPUT rows with the next block's norm1 affine, written as bf16 [M, D] -- the operand of the next
  // block's qkv projection (srhip_attn_block_fused), which saves that block's srhip_layernorm_fwd launch and its read of the residual stream
  bf16_t* ln_next;
  const float *gamma_n, *beta_n;
  float eps;
  int M, Hd, rows_per_sample;
  // PITCH variant of PROJ: logical row m of x, xo and ao lives at element m * pitch (one row per sample out of a [samples, tokens, D] buffer:
  // pitch = tokens * D); everything per row is the plain PROJ kernel's, so a row's result does not depend on the launch that carries it
  int pitch;
  // PLAN variant of PROJ (srhip_mlp_fused_proj_planned): plan[0] = n_mlp, plan[1 + q] = the sample that virtual sample q of the launch stands for
  // (a permutation of 0 .. nsamp - 1 with the n_mlp samples whose row_scale is not 0 first)
  const int* plan;
  int nsamp;
};

// DBG (tuning builds only, SRHIP_MLP_DEBUG): 1 = no GELU, 2 = no DMA / no vmcnt waits, 4 = no ds_reads, 8 = no MFMA
#ifdef SRHIP_TUNING
__device__ long long srhip_mlp_dbg[8 * 1024];
#define MDBG_T(i) do { if (threadIdx.x == 0 && blockIdx.x < 1024) srhip_mlp_dbg[8 * blockIdx.x + (i)] = wall_clock64(); } while (0)
#else
#define MDBG_T(i) do { } while (0)
#endif
// SPREAD: the ring refills are issued one per stage behind the stage's first MFMA half ("stage j asks for stage j + PD") instead of GS in a row
// right behind the group barrier.  An LDS-DMA instruction blocks its wave for ~100 cycles, and behind a barrier all eight waves -- both waves of
// every SIMD -- sit in that block together while the matrix pipe idles (measured on the producer / consumer kernel, profiles/r03_mlp_ps_*).
// PITCH: an instantiation of its own, so that the dense PROJ kernel keeps the code (and the register allocation) it has without the field
// PLAN (mlp_planned_kernel below): likewise.  Virtual row v of the launch is row v % rows_per_sample of sample plan[1 + v / rows_per_sample]: the rows' addresses and
// factors follow the map in the prologue and the epilogue, the main loop knows nothing of it.  Tiles below row n_mlp * rows_per_sample are
// "heavy" and run what the dense kernel runs; in the others every row has row_scale == 0 (the MLP branch dropped, vit.py:165): they stop
// after the projection -- no LN2, no b2 term, none of the fc1 / GELU / fc2 stages, whose products would all be multiplied by zero.
template <int D_, int DBG, int GS, bool PROJ = false, int SPREAD = 0, bool PITCH = false>
__global__ __launch_bounds__(512, 2) void mlp_fused_kernel(MlpArgs a) {
  constexpr bool PLAN = false;
#include "mlp_fused_body.h"
}
// the PLAN instantiation of the dense PROJ kernel with the SPREAD schedule: a kernel of its own name, so that the kernels above also keep theirs
template <int D_, int GS>
__global__ __launch_bounds__(512, 2) void mlp_planned_kernel(MlpArgs a) {
  constexpr int DBG = 0, SPREAD = 1;
  constexpr bool PROJ = true, PITCH = false, PLAN = true;
#include "mlp_fused_body.h"
}


__global__ void gelu_eval_kernel(const float* __restrict__ x, float* __restrict__ y_erf, float* __restrict__ y_poly, int n) {
  const int i = 2 * (blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const float a = x[i], b = i + 1 < n ? x[i + 1] : 0.f;
  const f32x2_t g = gelu_poly2(f32x2_t{a, b});
  y_erf[i] = gelu_erf(a); y_poly[i] = g[0];
  if (i + 1 < n) { y_erf[i + 1] = gelu_erf(b); y_poly[i + 1] = g[1]; }
}

}  // namespace

#ifdef SRHIP_TUNING
extern "C" int srhip_mlp_debug(long long* out_host, int n) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(srhip_mlp_dbg), (size_t)n * sizeof(long long)) == hipSuccess ? SR_OK : SR_EINVAL;
}
#endif
// The two GELU evaluations of the library on n values: y_erf = gelu_erf (exact-erf GELU to 1.5e-7, every path with a backward and every unfused
// epilogue), y_poly = gelu_poly2 (the transcendental-free form inside srhip_mlp_fused_proj) -- so that a test can pin the distance between them.
extern "C" int srhip_gelu_eval(const float* x, float* y_erf, float* y_poly, int n, void* stream) {
  if (!x || !y_erf || !y_poly || n <= 0) return SR_EINVAL;
  SR_LAUNCH(gelu_eval_kernel, dim3(cdiv((n + 1) / 2, 256)), dim3(256), 0, (hipStream_t)stream, x, y_erf, y_poly, n);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
extern "C" int srhip_mlp_fused(const float* x, float* x_out, const float* ln_gamma, const float* ln_beta, float eps, const void* W1,
                               const float* b1, const void* W2, const float* b2, const float* row_scale, int rows_per_sample,
                               int save_rows, void* save_ln2, void* save_pre, void* save_h, float* save_mean, float* save_rstd,
                               int M, int D, int Hd, void* stream) {
  if (!x || !x_out || !ln_gamma || !ln_beta || !W1 || !b1 || !W2 || !b2 || M <= 0) return SR_EINVAL;
  if (D != 384 || Hd < 128 || (Hd % RT) || Hd > 4096) return SR_EINVAL;          // ViT-S width; hidden in 128-wide chunks
  if (row_scale && rows_per_sample <= 0) return SR_EINVAL;
  if (save_rows < 0 || save_rows > M || (save_rows > 0 && (!save_ln2 || !save_pre || !save_h || !save_mean || !save_rstd))) return SR_EINVAL;
  if (((uintptr_t)x | (uintptr_t)x_out | (uintptr_t)W1 | (uintptr_t)W2 | (uintptr_t)ln_gamma | (uintptr_t)ln_beta | (uintptr_t)save_ln2 |
       (uintptr_t)save_pre | (uintptr_t)save_h) & 15)
    return SR_EINVAL;
  MlpArgs a;
  a.x = x; a.xo = x_out; a.gamma = ln_gamma; a.beta = ln_beta; a.b1 = b1; a.b2 = b2; a.row_scale = row_scale;
  a.s_ln2 = (bf16_t*)save_ln2; a.s_pre = (bf16_t*)save_pre; a.s_h = (bf16_t*)save_h; a.s_mean = save_mean; a.s_rstd = save_rstd;
  a.save_rows = save_rows;
  a.W1 = (const bf16_t*)W1; a.W2 = (const bf16_t*)W2; a.eps = eps; a.M = M; a.Hd = Hd;
  a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1;
  a.ao = nullptr; a.Wp = nullptr; a.bp = nullptr; a.row_scale1 = nullptr; a.ao_scaled = 0; a.ln_next = nullptr; a.gamma_n = a.beta_n = nullptr;
  a.pitch = D; a.plan = nullptr; a.nsamp = 0;
  const size_t smem = (size_t)NS * TILE_EL * sizeof(bf16_t) + (size_t)(Hd + 6 * D) * sizeof(float);
  void (*kern)(MlpArgs) = mlp_fused_kernel<384, 0, 4>;
#ifdef SRHIP_TUNING
  switch (SR_TUNE_ENV("SRHIP_MLP_DEBUG") ? atoi(SR_TUNE_ENV("SRHIP_MLP_DEBUG")) : 0) {
    case 1: kern = mlp_fused_kernel<384, 1, 4>; break;
    case 2: kern = mlp_fused_kernel<384, 2, 4>; break;
    case 3: kern = mlp_fused_kernel<384, 3, 4>; break;
    case 7: kern = mlp_fused_kernel<384, 7, 4>; break;
    case 11: kern = mlp_fused_kernel<384, 11, 4>; break;
    case 15: kern = mlp_fused_kernel<384, 15, 4>; break;
    case 100: kern = mlp_fused_kernel<384, 0, 2>; break;
    case 101: kern = mlp_fused_kernel<384, 0, 1>; break;
    default: break;
  }
#endif
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const int ntiles = cdiv(M, FBM);
  SR_LAUNCH(kern, dim3(min(ntiles, 256)), dim3(512), smem, (hipStream_t)stream, a);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

// Attention output projection + first residual + the whole MLP half of a block in ONE launch (rows without a backward):
//   x1 = x + row_scale1 * (ao Wp^T + bp);   x_out = x1 + row_scale2 * (fc2(GELU(fc1(LayerNorm(x1)))) + b2)
// (vit.py:163 tail: proj :105-106 + drop_path1 + residual, and :165).  Saves the proj GEMM launch and two reads + a write of the residual stream:
// x enters as the start value of the accumulators and x1 stays there.  ao_scaled != 0: ao already carries row_scale1 (only bp is scaled here).
// ln_next != NULL: also LayerNorm(x_out) with (next_gamma, next_beta) -- the next block's norm1 (vit.py:163) -- as bf16 [M, D].
// row_pitch == 0: rows packed at D (the dense kernel); otherwise the PITCH instantiation.  plan != NULL (row_pitch == 0): mlp_planned_kernel
static int mlp_fused_proj_launch(const float* x, float* x_out, const void* ao, const void* Wp, const float* bp, const float* row_scale1,
                                 int ao_scaled, const float* ln_gamma, const float* ln_beta, float eps, const void* W1, const float* b1, const void* W2,
                                 const float* b2, const float* row_scale2, int rows_per_sample, void* ln_next, const float* next_gamma,
                                 const float* next_beta, int M, int D, int Hd, int row_pitch, const int* plan, int nsamp, void* stream) {
  if (!x || !x_out || !ao || !Wp || !bp || !ln_gamma || !ln_beta || !W1 || !b1 || !W2 || !b2 || M <= 0) return SR_EINVAL;
  if (ln_next && (!next_gamma || !next_beta || ((uintptr_t)ln_next & 15))) return SR_EINVAL;
  if (D != 384 || Hd < 128 || (Hd % RT) || Hd > 4096) return SR_EINVAL;
  if ((row_scale1 || row_scale2) && rows_per_sample <= 0) return SR_EINVAL;
  if (((uintptr_t)x | (uintptr_t)x_out | (uintptr_t)ao | (uintptr_t)Wp | (uintptr_t)W1 | (uintptr_t)W2 | (uintptr_t)ln_gamma | (uintptr_t)ln_beta) & 15)
    return SR_EINVAL;
  MlpArgs a;
  a.x = x; a.xo = x_out; a.gamma = ln_gamma; a.beta = ln_beta; a.b1 = b1; a.b2 = b2; a.row_scale = row_scale2;
  a.s_ln2 = a.s_pre = a.s_h = nullptr; a.s_mean = a.s_rstd = nullptr; a.save_rows = 0;
  a.W1 = (const bf16_t*)W1; a.W2 = (const bf16_t*)W2; a.eps = eps; a.M = M; a.Hd = Hd;
  a.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1;
  a.ao = (const bf16_t*)ao; a.Wp = (const bf16_t*)Wp; a.bp = bp; a.row_scale1 = row_scale1; a.ao_scaled = ao_scaled;
  a.ln_next = (bf16_t*)ln_next; a.gamma_n = next_gamma; a.beta_n = next_beta; a.pitch = row_pitch ? row_pitch : D;
  a.plan = plan; a.nsamp = nsamp;
  const size_t smem = (size_t)NS * TILE_EL * sizeof(bf16_t) + (size_t)(Hd + 6 * D) * sizeof(float);
  // SRHIP_MLP_SPREAD=0: all GS refills of a group right behind its barrier (the round-2 schedule; A/B on one box: 104 -> 99.5 us per 105-image
  // launch, 1547 -> 1574 img/s on the step)
  static const int spread = SR_TUNE_ENV("SRHIP_MLP_SPREAD") ? atoi(SR_TUNE_ENV("SRHIP_MLP_SPREAD")) : 1;
  void (*kern)(MlpArgs) = spread ? mlp_fused_kernel<384, 0, 4, true, 1> : mlp_fused_kernel<384, 0, 4, true, 0>;
  if (row_pitch) kern = mlp_fused_kernel<384, 0, 4, true, 1, true>;
  if (plan) kern = mlp_planned_kernel<384, 4>;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  const int ntiles = cdiv(M, FBM);
  SR_LAUNCH(kern, dim3(min(ntiles, 256)), dim3(512), smem, (hipStream_t)stream, a);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_mlp_fused_proj(const float* x, float* x_out, const void* ao, const void* Wp, const float* bp, const float* row_scale1,
                                    int ao_scaled, const float* ln_gamma, const float* ln_beta, float eps, const void* W1, const float* b1, const void* W2,
                                    const float* b2, const float* row_scale2, int rows_per_sample, void* ln_next, const float* next_gamma,
                                    const float* next_beta, int M, int D, int Hd, void* stream) {
  return mlp_fused_proj_launch(x, x_out, ao, Wp, bp, row_scale1, ao_scaled, ln_gamma, ln_beta, eps, W1, b1, W2, b2, row_scale2, rows_per_sample, ln_next,
                               next_gamma, next_beta, M, D, Hd, 0, nullptr, 0, stream);
}

// srhip_mlp_fused_proj over M rows that lie row_pitch elements apart in x, x_out and ao (the class-token rows of a [samples, tokens, D] residual
// stream: M = samples, rows_per_sample = 1, row_pitch = tokens * D).  Rows in between are neither read nor written.
extern "C" int srhip_mlp_fused_proj_strided(const float* x, float* x_out, const void* ao, const void* Wp, const float* bp, const float* row_scale1,
                                            int ao_scaled, const float* ln_gamma, const float* ln_beta, float eps, const void* W1, const float* b1,
                                            const void* W2, const float* b2, const float* row_scale2, int rows_per_sample, void* ln_next,
                                            const float* next_gamma, const float* next_beta, int M, int D, int Hd, int row_pitch, void* stream) {
  if (row_pitch < D || (row_pitch % 8) != 0) return SR_EINVAL;     // rows must not overlap; 16-byte row starts of the fp32 and the bf16 operand
  if (ln_next && row_pitch != D) return SR_EINVAL;                 // the next block's norm1 rows are packed: only a dense launch writes them
  return mlp_fused_proj_launch(x, x_out, ao, Wp, bp, row_scale1, ao_scaled, ln_gamma, ln_beta, eps, W1, b1, W2, b2, row_scale2, rows_per_sample, ln_next,
                               next_gamma, next_beta, M, D, Hd, row_pitch, nullptr, 0, stream);
}

// srhip_mlp_fused_proj whose rows follow a DropPath plan row (srhip_vit_droppath_plan): virtual row v of the launch is row v % rows_per_sample of
// sample plan_row[1 + v / rows_per_sample], in x, x_out, ao and ln_next; the two factors are looked up by that sample.  Tiles (128 virtual rows)
// that start at or beyond row plan_row[0] * rows_per_sample hold only samples whose row_scale2 is 0 and stop after the projection.
extern "C" int srhip_mlp_fused_proj_planned(const float* x, float* x_out, const void* ao, const void* Wp, const float* bp, const float* row_scale1,
                                            int ao_scaled, const float* ln_gamma, const float* ln_beta, float eps, const void* W1, const float* b1,
                                            const void* W2, const float* b2, const float* row_scale2, int rows_per_sample, void* ln_next,
                                            const float* next_gamma, const float* next_beta, int M, int D, int Hd, const int* plan_row, int B,
                                            void* stream) {
  if (!plan_row || ((uintptr_t)plan_row & 3) || B <= 0 || rows_per_sample <= 0 || !row_scale2) return SR_EINVAL;
  if ((long long)B * rows_per_sample != (long long)M) return SR_EINVAL;
  return mlp_fused_proj_launch(x, x_out, ao, Wp, bp, row_scale1, ao_scaled, ln_gamma, ln_beta, eps, W1, b1, W2, b2, row_scale2, rows_per_sample, ln_next,
                               next_gamma, next_beta, M, D, Hd, 0, plan_row, B, stream);
}
