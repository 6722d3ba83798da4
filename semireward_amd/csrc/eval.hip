// Evaluation tail (semilearn/core/algorithmbase.py:377-457) as ONE launch per batch that accumulates on the device: per row the cross
// entropy F.cross_entropy(ignore_index=-1) sees and the argmax torch.max(logits, dim=-1)[1] returns; per batch one count in the confusion
// matrix per row and one fp64 term of the reference's `total_loss += loss.item() * num_batch`.  The host reads (C + 1) * C integers and the
// state once, at the end of the evaluation, instead of every batch's logits.
//
// One wave per row, as criterions.hip: a row of C <= 1024 logits is read ONCE (16-byte loads when base and stride allow) and lives in
// registers through the max / argmax and the sum sweeps; longer rows are re-read (they hit L2).  The label's own logit z[y] is one more
// scalar read of a line the row load just brought in.  Row arithmetic is fp32.  pred_out is written for every row, also one whose label
// is out of range: it is an output, not an accumulator.
// The launch is ONE workgroup of 16 waves (wave w takes rows w, w + 16, ...): every wave adds its rows' losses in row order in fp64,
// thread 0 adds the 16 partial sums in wave order and updates the state -- no float atomics, and launches of one stream are ordered, so
// two runs give the same bits.  Evaluation batches are small (eval_batch_size rows); one workgroup keeps the batch reduction in the
// launch without a scratch buffer.  The confusion counts are integer atomics: integer sums do not depend on the order.
#include <limits.h>

#include "common.h"
#include "srhip.h"

// op by op, no fused multiply-add: the 16-byte and the scalar instantiations must give the same bits
#pragma clang fp contract(off)

namespace {

constexpr int NIT = 4;                    // register-resident chunks: 4 x (64 lanes x 4 floats) = 1024 columns
constexpr int WAVES = 16;

struct EvalState { double loss_sum, nll_sum; long long rows, kept; };      // srhip.h: state of srhip_eval_accumulate

struct EvalArgs {
  const float* logits; long long ld;
  const long long* y;
  int* confusion; EvalState* state;
  long long* pred_out; long long row_offset;
  int* label_err;
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

template <bool CACHED, typename Fn> __device__ __forceinline__ void each_chunk(int lane, int C, Fn&& f) {
  if constexpr (CACHED) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) f(it, it * 256 + lane * 4);
  } else {
    for (int c0 = lane * 4; c0 < C; c0 += 256) f(0, c0);
  }
}

// the order numpy.argmax / torch.argmax use: a NaN is maximal, and among equals (two NaNs, two equal values) the lower column wins
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {
  const bool n = v != v, bn = bv != bv;
  if (n != bn) return n;
  if (n || v == bv) return i < bi;
  return v > bv;
}

// max (NaNs ignored, for the shift), argmax and sum_c exp(z_c - max) of one row; the same values in every lane
template <bool VEC, bool CACHED>
__device__ __forceinline__ void row_stats(const float* __restrict__ z, int C, int lane, float& mx, float& s, int& pred) {
  f32x4_t zr[NIT];
  if constexpr (CACHED) each_chunk<true>(lane, C, [&](int it, int c0) { zr[it] = ld4<VEC>(z, c0, C); });
  auto Z = [&](int it, int c0) -> f32x4_t { if constexpr (CACHED) return zr[it]; else return ld4<VEC>(z, c0, C); };

  mx = -INFINITY;
  float bv = -INFINITY;
  int bi = INT_MAX;                       // a lane without a column loses against every column, an all -inf row gives column 0
  each_chunk<CACHED>(lane, C, [&](int it, int c0) {
    const f32x4_t zv = Z(it, c0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < C) {
        mx = fmaxf(mx, zv[j]);
        if (better(zv[j], c0 + j, bv, bi)) { bv = zv[j]; bi = c0 + j; }
      }
  });
  mx = wave_max(mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {      // `better` is a total order on (value, column): the butterfly ends with one winner in all lanes
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  pred = bi;
  float a = 0.f;
  each_chunk<CACHED>(lane, C, [&](int it, int c0) {
    const f32x4_t zv = Z(it, c0);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (c0 + j < C) a += expf(zv[j] - mx);
  });
  s = wave_sum(a);
}

template <bool VEC, bool CACHED> __global__ __launch_bounds__(WAVES * 64) void eval_accumulate_kernel(EvalArgs a) {
  __shared__ double part[WAVES];
  __shared__ int seen_s[WAVES], kept_s[WAVES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int C = a.C;
  double acc = 0.0;
  int seen = 0, kept = 0;
  for (int row = wave; row < a.B; row += WAVES) {
    const float* z = a.logits + (size_t)row * a.ld;
    float mx, s;
    int pred;
    row_stats<VEC, CACHED>(z, C, lane, mx, s, pred);
    const long long y = a.y[row];
    if (a.pred_out && lane == 0) a.pred_out[a.row_offset + row] = pred;
    if (y < -1 || y >= (long long)C) {                          // F.cross_entropy raises: recorded, the row reaches no accumulator
      if (lane == 0) atomicOr(a.label_err, 16);
      continue;
    }
    ++seen;
    if (lane == 0) atomicAdd(a.confusion + (size_t)(y < 0 ? C : (int)y) * C + pred, 1);
    if (y >= 0) {                                               // ignore_index = -1: counted in row C, kept out of the loss
      acc += (double)(logf(s) - (z[y] - mx));
      ++kept;
    }
  }
  if (lane == 0) { part[wave] = acc; seen_s[wave] = seen; kept_s[wave] = kept; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    int n = 0, k = 0;
    for (int w = 0; w < WAVES; ++w) { tot += part[w]; n += seen_s[w]; k += kept_s[w]; }
    EvalState* st = a.state;
    st->loss_sum += tot / (double)(k > 0 ? k : 1) * (double)a.B;      // loss.item() * num_batch (algorithmbase.py:413); 0 for a batch without kept rows
    st->nll_sum += tot;
    st->rows += n;
    st->kept += k;
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <bool VEC> void launch(const EvalArgs& a, hipStream_t s) {
  if (a.C <= NIT * 256) SR_LAUNCH((eval_accumulate_kernel<VEC, true>), dim3(1), dim3(WAVES * 64), 0, s, a);
  else SR_LAUNCH((eval_accumulate_kernel<VEC, false>), dim3(1), dim3(WAVES * 64), 0, s, a);
}

}  // namespace

extern "C" int srhip_eval_accumulate(const float* logits, long long ld, const long long* y, int* confusion, void* state, long long* pred_out,
                                     long long row_offset, int B, int C, void* stream) {
  if (B <= 0 || B > 65535 || C <= 0 || !logits || !y || !confusion || !state || ld < C || row_offset < 0) return SR_EINVAL;
  if (((uintptr_t)state & 7u) != 0) return SR_EINVAL;
  int* err = sr_label_err_ptr();
  if (!err) return SR_ELAUNCH;
  const EvalArgs a{logits, ld, y, confusion, (EvalState*)state, pred_out, row_offset, err, B, C};
  if (al16(logits) && ld % 4 == 0) launch<true>(a, (hipStream_t)stream);
  else launch<false>(a, (hipStream_t)stream);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
