// Pillow-exact bilinear resize of a uint8 HWC image stack: the transforms.Resize(crop_size) that opens transform_weak / transform_strong /
// transform_val of every USB CV dataset, applied ONCE to the stored array when a dataset is put on the device (data/device_loader.py).
//
// Replaces (host CPU, per sample and per epoch in the reference):
//   semilearn/datasets/cv_datasets/eurosat.py:66,76,87   cifar.py:35,43,52   stl10.py:43,51,60
//   transforms.Resize(S) on a PIL image = Image.resize((S, S), BILINEAR) = Pillow's ImagingResample for 8-bit images
// Pillow computes per output pixel a window [xmin, xmin + n) and n triangle-filter weights in float64, normalises them and converts them to
// 22-bit fixed point; that part depends only on (H0, S) and is done once on the host (data/resize.py: resize_tables, CPython floats are the C
// doubles).  What is left is integer only: a horizontal pass into a uint8 intermediate, then a vertical pass, each
// clip8((2^21 + sum pixel * k) >> 22).  One 256-thread workgroup per image; the intermediate is a global scratch plane (L2 resident).
#include "common.h"
#include "srhip.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ unsigned char clip8(int v) {
  v >>= PRECISION_BITS;                         // arithmetic shift, as Pillow's table lookup of in >> PRECISION_BITS
  return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__global__ __launch_bounds__(256) void resize_bilinear_u8_kernel(const unsigned char* __restrict__ src, int H0, int S, int ksize,
                                                                const int* __restrict__ bounds, const int* __restrict__ kk,
                                                                unsigned char* __restrict__ tmp, unsigned char* __restrict__ dst) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned char* im = src + (size_t)b * H0 * H0 * 3;
  unsigned char* T = tmp + (size_t)b * H0 * S * 3;
  unsigned char* D = dst + (size_t)b * S * S * 3;
  // ---- horizontal pass: T[y][x][c], y < H0, x < S
  for (int p = tid; p < H0 * S * 3; p += 256) {
    const int c = p % 3, q = p / 3, y = q / S, x = q - y * S;
    const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
    int ss = 1 << (PRECISION_BITS - 1);
    if (xmin >= 0 && n >= 0 && n <= ksize && xmin + n <= H0) {      // (a table that does not belong to (H0, S) must not read out of bounds)
      const unsigned char* row = im + ((size_t)y * H0 + xmin) * 3 + c;
      const int* k = kk + (size_t)x * ksize;
      for (int i = 0; i < n; ++i) ss += (int)row[i * 3] * k[i];
    }
    T[p] = clip8(ss);
  }
  __syncthreads();
  // ---- vertical pass: D[y][x][c], y < S, x < S
  for (int p = tid; p < S * S * 3; p += 256) {
    const int c = p % 3, q = p / 3, y = q / S, x = q - y * S;
    const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
    int ss = 1 << (PRECISION_BITS - 1);
    if (ymin >= 0 && n >= 0 && n <= ksize && ymin + n <= H0) {
      const unsigned char* col = T + ((size_t)ymin * S + x) * 3 + c;
      const int* k = kk + (size_t)y * ksize;
      for (int i = 0; i < n; ++i) ss += (int)col[(size_t)i * S * 3] * k[i];
    }
    D[p] = clip8(ss);
  }
}

// H0 == S: Pillow skips both passes and returns a copy of the image
__global__ __launch_bounds__(256) void copy_u8_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}

}  // namespace

extern "C" int srhip_resize_bilinear_u8(const unsigned char* src, int N, int H0, int W0, unsigned char* dst, int S, const int* bounds,
                                        const int* coefs, int ksize, unsigned char* tmp, void* stream) {
  if (!src || !dst || N <= 0 || H0 <= 0 || S <= 0 || H0 != W0) return SR_EINVAL;
  const long long big = H0 > S ? H0 : S;
  if (big * big * 3 > (1LL << 30)) return SR_EINVAL;                                // per-image index arithmetic is int (H0 * S * 3, S * S * 3)
  if (H0 == S) {
    const size_t n = (size_t)N * S * S * 3;
    const size_t blocks = (n + 255) / 256;
    SR_LAUNCH(copy_u8_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, src, dst, n);
    SR_CHECK_LAUNCH();
    return SR_OK;
  }
  if (!bounds || !coefs || !tmp || ksize <= 0) return SR_EINVAL;
  SR_LAUNCH(resize_bilinear_u8_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, src, H0, S, ksize, bounds, coefs, tmp, dst);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
