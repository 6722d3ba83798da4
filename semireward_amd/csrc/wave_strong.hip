// One effect slot of the device-made strong waveform view (``device_audio_strong: True``, data/device_audio.py): every row of a batch goes
// through ONE of copy / gain / resample / reverb, read from the resident clip store (slot 0) or from the scratch rows the previous slot wrote
// (slot 1), written to scratch rows of a fixed pitch.  The chain is the engine's own -- it keeps the STRUCTURE of the reference's
// WaveformTransforms (semilearn/datasets/audio_datasets/datasetbase.py:12-39: two effects drawn with replacement from gain / pitch / speed /
// reverb, applied to the whole clip before random_subsample) and its draw distributions, not sox's filters; configs/README.md lists the
// deviations.  tests/_wave_strong_cases.py restates every effect in float64 numpy: that restatement is the specification.
//
// One 1024-thread workgroup per row (16 waves, four per SIMD: a row is one CU's work, B <= 65535 rows); rows of different ops share the launch.
// No atomics and a fixed summation order everywhere: equal inputs give equal bits.
//   copy      16-byte loads where the source row is 16-byte aligned (store rows and scratch rows are), 16-byte stores.
//   gain      sox ``gain -n``: peak = max |x| (exact: a maximum has no rounding), out = clamp(x * (g / peak), -1, 1) with the quotient and the
//             product in fp64 and ONE fp32 rounding, so that an element is within 0.5 ulp of the product with the fp32 g the host passes
//             (itself within 1 ulp of the float64 product with 10^(att / 20)).  peak == 0 copies.
//   resample  a windowed-sinc gather, serves ``speed`` and ``pitch``.  Output j sits at input position j * step, a 32.32 fixed-point product
//             in 64-bit integers (an fp32 j * s has no fractional bits left at the lengths a 30 s clip reaches); the weights are fp32 from
//             the fraction: h(u) = c sinc(c u) (0.5 + 0.5 cos(pi u / T)), c = min(1, 2^32 / step), T = 16 / c, taps k ascending over
//             |i0 + f - k| < T inside the row (at most 66, no renormalisation at the edges).  The trigonometric factors are split into a
//             per-row table over the integer part of the tap's distance and four evaluations per output (resample_row).  The input window
//             is read DIRECTLY from global memory: neighbouring lanes' windows overlap in all but one sample, so the loads of a wave fall
//             into a few cache lines the CU's L1 already holds; staging through LDS would add a barrier per tile to save loads that do not
//             miss.  step == 2^32 copies bit for bit.
//   reverb    the public-domain Freeverb network, mono, wet only: input gain 0.015, eight parallel lowpass-feedback combs (feedback 0.84,
//             damping 0.2), four series allpasses (0.5), output scale 3.  The only serial part, evaluated in chunks of C = the shortest of
//             the 12 delays: inside a chunk every delayed read is of an earlier chunk, so the samples of a chunk are independent.  The one
//             recursion inside a comb, the damping lowpass st[n] = 0.8 y[n] + 0.2 st[n - 1], is evaluated as its own first 24 terms
//             (0.8 sum_k 0.2^k y[n - k], Horner from the oldest: the remainder is below 0.2^24 = 1.7e-17 of the signal).  Threads are laid
//             out [8 combs][128 samples]: phase A computes each comb's 24-term state and new delay-line sample and parks the comb outputs in
//             LDS, one barrier, phase B (128 threads) adds the eight outputs in comb order and runs the four allpasses.  The comb output
//             buffer is double-buffered, so one barrier per chunk is enough, and a chunk's input samples are loaded while the chunk
//             before it is computed.  A chunk costs 1.15 us whatever its arithmetic (781 chunks, 902 us for 64 000 samples at 16 kHz;
//             983 us with the load inside the chunk): the LDS round trips of phase A, the barrier, and the four dependent LDS round trips
//             of phase B follow each other (profiles/wave_strong.txt says what a faster form needs).  Delay lines are rings in LDS of D + 23 + C (comb) and D + C
//             (allpass) floats, zero at the start: a slot read before it was written holds the zero the network's empty state prescribes.
#include "common.h"
#include "srhip.h"

namespace {

constexpr int NT = 1024, NWAVES = NT / 64, SX = 128, FIR = 24;
constexpr int CHUNK_IT = 2;                            // samples of a chunk a thread serves: chunks of up to CHUNK_IT * SX samples
constexpr int RESAMPLE_TAB = 72;                       // float4 entries of the resample's per-row table (2 * 34 + 1 are used at most)
constexpr unsigned long long ONE = 1ull << 32;
constexpr int LDS_BUDGET = 64 * 1024 - 256;            // dynamic LDS of one workgroup without opting in to more, less the static words

struct wave_delays {
  int d[12];                                           // eight combs, four allpasses, in samples
};

// floats of LDS the reverb needs for these delays; C = the chunk
static inline long reverb_lds_floats(const int* d, int* chunk) {
  int C = d[0];
  for (int i = 1; i < 12; ++i) C = d[i] < C ? d[i] : C;
  long tot = 16L * C;
  for (int i = 0; i < 8; ++i) tot += (long)d[i] + (FIR - 1) + C;
  for (int i = 8; i < 12; ++i) tot += (long)d[i] + C;
  *chunk = C;
  return tot;
}

__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
#pragma unroll
  for (int i = 1; i < NWAVES; ++i) m = fmaxf(m, red[i]);
  return m;
}

// samples t0 .. t0 + 3 of a row of n samples, zero past its end
__device__ __forceinline__ f32x4_t load4(const float* __restrict__ p, int t0, int n, bool aligned) {
  if (aligned && t0 + 4 <= n) return *reinterpret_cast<const f32x4_t*>(p + t0);
  f32x4_t v;
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = t0 + j < n ? p[t0 + j] : 0.f;
  return v;
}

// o[t0 .. t0 + 3] = v, nothing at or past m (o is 16-byte aligned, t0 a multiple of 4)
__device__ __forceinline__ void store4(float* __restrict__ o, int t0, int m, f32x4_t v) {
  if (t0 + 4 <= m) {
    *reinterpret_cast<f32x4_t*>(o + t0) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (t0 + j < m) o[t0 + j] = v[j];
  }
}

__device__ __forceinline__ void copy_row(const float* __restrict__ p, int n, float* __restrict__ o, int m, int tid) {
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  for (int t0 = 4 * tid; t0 < m; t0 += 4 * NT) store4(o, t0, m, load4(p, t0, n, aligned));
}

__device__ __forceinline__ void gain_row(const float* __restrict__ p, int n, float* __restrict__ o, int m, float g, int tid, float* red) {
  const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  float pk = 0.f;
  for (int t0 = 4 * tid; t0 < n; t0 += 4 * NT) {
    const f32x4_t v = load4(p, t0, n, aligned);
    pk = fmaxf(fmaxf(pk, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
  }
  pk = block_max(pk, red);
  if (pk == 0.f) {
    copy_row(p, n, o, m, tid);
    return;
  }
  const double scale = (double)g / (double)pk;
  for (int t0 = 4 * tid; t0 < m; t0 += 4 * NT) {
    f32x4_t v = load4(p, t0, n, aligned);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fminf(fmaxf((float)((double)v[j] * scale), -1.f), 1.f);
    store4(o, t0, m, v);
  }
}

// A tap sits at u = d + f with d an integer and |f| <= 1/2 (the position's fraction, taken to the NEAREST input sample), so the two
// trigonometric factors of its weight split by the angle-addition formulas into a part that depends on d alone -- a table of at most 69
// entries {sin(pi c d), cos(pi c d), sin(pi d / T), cos(pi d / T)}, computed once per row in fp64 and rounded -- and a part that depends on f
// alone: four fp32 evaluations per OUTPUT instead of two per TAP.  With the nearest split a small |u| occurs only at d = 0, whose table
// entry is exactly {0, 1, 0, 1}: the sinc's numerator is then sin(pi c f) itself and keeps its relative accuracy where it is divided by a
// small pi c u.
__device__ __forceinline__ void resample_row(const float* __restrict__ p, int n, float* __restrict__ o, int m, unsigned long long step, int tid,
                                             f32x4_t* __restrict__ tab) {
  const double s = (double)step * (1.0 / 4294967296.0), wide = s > 1.0 ? s : 1.0, cd = 1.0 / wide, invTd = cd * (1.0 / 16.0);
  const float c = (float)cd, T = (float)(16.0 * wide), invT = (float)invTd, pic = (float)(3.14159265358979323846 * cd);
  const int Ti = (int)T + 1;                           // |d + f| < T with |f| <= 1/2 needs |d| <= Ti  (Ti <= 34: RESAMPLE_TAB entries)
  for (int i = tid; i <= 2 * Ti; i += NT) {
    const double d = (double)(i - Ti);
    tab[i] = f32x4_t{(float)sinpi(cd * d), (float)cospi(cd * d), (float)sinpi(invTd * d), (float)cospi(invTd * d)};
  }
  __syncthreads();
  for (int j = tid; j < m; j += NT) {
    const unsigned long long pos = (unsigned long long)j * step;
    float f = (float)(unsigned)(pos & 0xffffffffu) * 2.3283064365386963e-10f;
    const int up = f >= 0.5f;
    const long long i0 = (long long)(pos >> 32) + up;  // the nearest input sample; k = i0 - d
    f -= (float)up;                                    // (exact: f - 1 with f in [1/2, 1])
    const float sf = sinpif(c * f), cf = cospif(c * f), sw = sinpif(f * invT), cw = cospif(f * invT);
    const int dhi = (int)min(i0, (long long)Ti), dlo = (int)max(i0 - (n - 1), (long long)-Ti);      // 0 <= k <= n - 1
    const float* __restrict__ q = p + i0;
    float acc = 0.f;
    for (int d = dhi; d >= dlo; --d) {                 // k ascending
      const float u = (float)d + f;
      if (fabsf(u) < T) {
        const f32x4_t e = tab[d + Ti];
        const float sn = fmaf(e[0], cf, e[1] * sf), wn = fmaf(e[3], cw, -(e[2] * sw));
        const float sinc = u == 0.f ? 1.f : sn / (pic * u);
        acc = fmaf(q[-d], c * sinc * (0.5f + 0.5f * wn), acc);
      }
    }
    o[j] = acc;
  }
}

__device__ __forceinline__ void reverb_row(const float* __restrict__ p, int n, float* __restrict__ o, int m, const wave_delays& dl, int tid,
                                           float* __restrict__ lds) {
  const int x = tid & (SX - 1), y = tid / SX;         // the comb this thread serves in phase A, and its sample lane
  int C = dl.d[0];
#pragma unroll
  for (int i = 1; i < 12; ++i) C = min(C, dl.d[i]);
  int off = 0, cD = 0, cR = 0, cOff = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int R = dl.d[i] + (FIR - 1) + C;
    if (i == y) cD = dl.d[i], cR = R, cOff = off;
    off += R;
  }
  int aR[4], aOff[4], aBase[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    aR[a] = dl.d[8 + a] + C, aOff[a] = off, aBase[a] = 0;
    off += aR[a];
  }
  float* __restrict__ part = lds + off;               // [2][8][C]: the comb outputs of the chunk in flight and of the next
  for (int i = tid; i < off + 16 * C; i += NT) lds[i] = 0.f;
  __syncthreads();
  float* __restrict__ ring = lds + cOff;
  int cBase = 0, parity = 0;                           // ring slot of the chunk's first sample
  const int last = min(n, m);
  float xin[CHUNK_IT], xnext[CHUNK_IT];                // the chunk's input samples, loaded one chunk ahead: the barrier never waits for memory
#pragma unroll
  for (int it = 0; it < CHUNK_IT; ++it) xin[it] = x + it * SX < min(C, last) ? p[x + it * SX] : 0.f;
  for (int n0 = 0; n0 < m; n0 += C) {
    const int cn = min(C, m - n0);
    float* __restrict__ mine = part + (parity * 8 + y) * C;
#pragma unroll
    for (int it = 0; it < CHUNK_IT; ++it) {
      const int t = x + it * SX;
      xnext[it] = t < C && n0 + C + t < last ? p[n0 + C + t] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < CHUNK_IT; ++it) {            // phase A: comb y, sample n0 + t
      const int t = x + it * SX;
      if (t >= cn) break;
      int wp = cBase + t;
      if (wp >= cR) wp -= cR;
      int rp = wp - cD - (FIR - 1);                    // the slot of w[n - D - 23]: a sample of an earlier chunk (D >= C), or still zero
      if (rp < 0) rp += cR;
      float st = 0.f, v = 0.f;
#pragma unroll
      for (int k = 0; k < FIR; ++k) {
        v = ring[rp];
        st = fmaf(0.2f, st, v);
        if (++rp == cR) rp = 0;
      }
      ring[wp] = fmaf(0.84f, 0.8f * st, 0.015f * xin[it]);
      mine[t] = v;                                     // the comb's output: what it stored D samples ago
    }
    __syncthreads();
    if (y == 0) {
      const float* __restrict__ q = part + parity * 8 * C;
      for (int t = x; t < cn; t += SX) {               // phase B: sum in comb order, four allpasses
        float in = q[t];
#pragma unroll
        for (int i = 1; i < 8; ++i) in += q[i * C + t];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          float* __restrict__ ar = lds + aOff[a];
          int wp = aBase[a] + t;
          if (wp >= aR[a]) wp -= aR[a];
          int rp = wp - dl.d[8 + a];
          if (rp < 0) rp += aR[a];
          const float b = ar[rp];
          ar[wp] = fmaf(0.5f, b, in);
          in = b - in;
        }
        o[n0 + t] = 3.f * in;
      }
    }
    cBase += C;
    if (cBase >= cR) cBase -= cR;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      aBase[a] += C;
      if (aBase[a] >= aR[a]) aBase[a] -= aR[a];
    }
    parity ^= 1;
#pragma unroll
    for (int it = 0; it < CHUNK_IT; ++it) xin[it] = xnext[it];
  }
}

__global__ __launch_bounds__(NT) void wave_effect_kernel(const float* __restrict__ store, const long long* __restrict__ row_off,
                                                         const int* __restrict__ row_len, int n_rows, const long long* __restrict__ src_row,
                                                         const int* __restrict__ op, const long long* __restrict__ param,
                                                         const int* __restrict__ dst_len, float* __restrict__ dst, int pitch, wave_delays dl) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float red[NWAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long r = src_row[b];
  if (r < 0 || r >= n_rows) return;                    // (the entry and the wrapper refuse these on the host: nothing is read, nothing written)
  const int n = row_len[r], m = min(dst_len[b], pitch), e = op[b];
  if (n <= 0 || m <= 0) return;
  const float* __restrict__ p = store + row_off[r];
  float* __restrict__ o = dst + (size_t)b * pitch;
  const unsigned long long step = (unsigned long long)param[b];
  if (e == SR_WAVE_COPY || (e == SR_WAVE_RESAMPLE && step == ONE)) {
    copy_row(p, n, o, m, tid);
  } else if (e == SR_WAVE_GAIN) {
    gain_row(p, n, o, m, __uint_as_float((unsigned)param[b]), tid, red);
  } else if (e == SR_WAVE_RESAMPLE) {
    if (step >= (ONE >> 1) && step <= (ONE << 1)) resample_row(p, n, o, m, step, tid, reinterpret_cast<f32x4_t*>(lds));
  } else if (e == SR_WAVE_REVERB) {
    reverb_row(p, n, o, m, dl, tid, lds);
  }
}

}  // namespace

extern "C" int srhip_wave_effect(const float* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row,
                                 const int* op, const long long* param, const int* dst_len, int B, float* dst, int pitch, const int* host_op,
                                 const long long* host_param, const int* host_dst_len, const int* delays12, void* stream) {
  if (!store || !row_off || !row_len || !src_row || !op || !param || !dst_len || !dst || !host_op || !host_param || !host_dst_len || !delays12)
    return SR_EINVAL;
  if (n_rows <= 0 || B <= 0 || B > 65535 || pitch <= 0 || (pitch & 3) || (reinterpret_cast<uintptr_t>(dst) & 15)) return SR_EINVAL;
  if (reinterpret_cast<uintptr_t>(store) & 3) return SR_EINVAL;
  for (int b = 0; b < B; ++b) {
    if (host_op[b] < SR_WAVE_COPY || host_op[b] > SR_WAVE_REVERB || host_dst_len[b] <= 0 || host_dst_len[b] > pitch) return SR_EINVAL;
    if (host_op[b] == SR_WAVE_RESAMPLE && (host_param[b] < (long long)(ONE >> 1) || host_param[b] > (long long)(ONE << 1))) return SR_EINVAL;
  }
  wave_delays dl;
  for (int i = 0; i < 12; ++i) {
    if (delays12[i] <= 0 || delays12[i] > LDS_BUDGET / 4) return SR_EINVAL;
    dl.d[i] = delays12[i];
  }
  int chunk;
  const long floats = reverb_lds_floats(dl.d, &chunk);
  if (floats * 4 > LDS_BUDGET || chunk > CHUNK_IT * SX) return SR_EINVAL;
  const long bytes = floats * 4 > RESAMPLE_TAB * 16 ? floats * 4 : RESAMPLE_TAB * 16;      // the delay lines, or the resample's table
  SR_LAUNCH(wave_effect_kernel, dim3(B), dim3(NT), (unsigned)bytes, (hipStream_t)stream, store, row_off, row_len, n_rows, src_row, op, param,
            dst_len, dst, pitch, dl);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
