// One view of a batch of waveforms from the device-resident clip store (data/device_audio.py, ``device_audio: True``): crop, zero-pad to S
// samples and, when asked, the zero-mean / unit-variance normalisation of transformers' Wav2Vec2FeatureExtractor -- one launch per view.
//
// Replaces (host CPU, per sample and per batch in the reference):
//   semilearn/datasets/utils.py:177-183                      random_subsample: wav[off : off + L]  (the offset is drawn on the host, per epoch)
//   semilearn/datasets/collactors/audio_collactor.py:61-83   Wav2Vec2FeatureExtractor(padding=..., truncation=True): pad with zeros, then
//   transformers' zero_mean_unit_var_norm without an attention mask: (x - x.mean()) / sqrt(x.var() + 1e-7) over the PADDED vector
//
// One 256-thread workgroup per output row (B <= 65535 rows; 8 rows of 64 000 samples in front of a ~20 ms step: not a throughput kernel).
// The window's first sample sits at an arbitrary float of the store, so the two statistics passes peel up to three head samples, read the
// body as 16-byte aligned float4 and peel the tail; the output row is 16-byte aligned and written as float4 (the last, partial quad of a
// row whose S is no multiple of 4 as scalars: columns S .. ldo are never touched).  The statistics are accumulated in fp64 -- mean first,
// then the centred second moment, the S - n padded zeros counted analytically -- each thread over a fixed stride, the wave by a butterfly,
// the four waves through LDS in wave order: no atomics, the same inputs give the same bits.  An element is
// fp32((double(v) - m) * (1 / sqrt(var + 1e-7))): one fp32 rounding of a float64 value.
#include "common.h"
#include "srhip.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the workgroup's 256 threads, the same value in every thread; ``red`` holds one double per wave
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  __syncthreads();                                   // (the previous use of ``red`` has been read)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// f(v) summed over p[0 .. n): ``head`` scalars up to the first 16-byte boundary, aligned float4, scalar tail
template <typename F>
__device__ __forceinline__ double window_sum(const float* __restrict__ p, int n, int head, F f) {
  const int tid = threadIdx.x;
  const int nb = (n - head) >> 2, tail0 = head + 4 * nb;
  double acc = 0.0;
  if (tid < head) acc += f(p[tid]);
  const f32x4_t* __restrict__ q = reinterpret_cast<const f32x4_t*>(p + head);
  for (int i = tid; i < nb; i += 256) {
    const f32x4_t v = q[i];
    acc += (f(v[0]) + f(v[1])) + (f(v[2]) + f(v[3]));
  }
  if (tid < n - tail0) acc += f(p[tail0 + tid]);
  return acc;
}

__global__ __launch_bounds__(256) void wave_view_kernel(const float* __restrict__ store, const long long* __restrict__ row_off,
                                                        const int* __restrict__ row_len, int n_rows, const long long* __restrict__ src_row,
                                                        const int* __restrict__ crop_off, int S, int normalize, float* __restrict__ out,
                                                        int ldo) {
  __shared__ double red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long r = src_row[b];
  int n = 0;                                          // samples of the window that exist; a row or an offset outside the store: none
  const float* p = store;
  if (r >= 0 && r < n_rows) {
    const int len = row_len[r], c = crop_off[b];
    if (len > 0 && c >= 0 && c < len) {
      n = min(len - c, S);
      p = store + row_off[r] + c;
    }
  }
  const int mis = (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3);
  const int head = min((4 - mis) & 3, n);
  double m = 0.0, rs = 1.0;
  if (normalize) {
    m = block_sum_f64(window_sum(p, n, head, [](float v) { return (double)v; }), red) / (double)S;
    const double c2 = block_sum_f64(window_sum(p, n, head, [m](float v) { const double d = (double)v - m; return d * d; }), red);
    const double var = (c2 + (double)(S - n) * (m * m)) / (double)S;
    rs = 1.0 / sqrt(var + 1e-7);
  }
  float* __restrict__ o = out + (size_t)b * ldo;
  const bool aligned = mis == 0;
  for (int q = tid; 4 * q < S; q += 256) {
    const int t0 = 4 * q;
    f32x4_t v;
    if (aligned && t0 + 4 <= n) {
      v = *reinterpret_cast<const f32x4_t*>(p + t0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = t0 + j < n ? p[t0 + j] : 0.f;
    }
    if (normalize) {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (float)(((double)v[j] - m) * rs);
    }
    if (t0 + 4 <= S) {
      *reinterpret_cast<f32x4_t*>(o + t0) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < S) o[t0 + j] = v[j];
    }
  }
}

}  // namespace

extern "C" int srhip_wave_view(const float* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row,
                               const int* crop_off, int B, int S, int normalize, float* out, int ldo, void* stream) {
  if (!store || !row_off || !row_len || !src_row || !crop_off || !out) return SR_EINVAL;
  if (n_rows <= 0 || B <= 0 || B > 65535 || S <= 0 || S > (1 << 30) || ldo < S || (ldo & 3) || (reinterpret_cast<uintptr_t>(out) & 15)) return SR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(store) & 3) || (normalize != 0 && normalize != 1)) return SR_EINVAL;
  SR_LAUNCH(wave_view_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, store, row_off, row_len, n_rows, src_row, crop_off, S, normalize,
            out, ldo);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
