// One view of a batch of token sequences from the device-resident token store (data/device_tokens.py, ``device_tokens: True``): gather the
// rows, truncate to L, right-pad with pad_id, widen int32 -> int64 and write the lengths -- one launch per view.
//
// Replaces (host CPU, per step in the reference):
//   semilearn/datasets/collactors/nlp_collactor.py:49-61    tokenizer(text, max_length, truncation=True, padding=False) of every sentence, every step
//   semilearn/datasets/collactors/nlp_collactor.py:63-110   tokenizer.pad(padding=True): right-pad with [PAD] to the batch's longest row
// and, on this side, TokenBatch.from_dict's cast / copy of the padded batch and the srhip_mask_lengths launch that recovers the lengths.
//
// One 256-thread workgroup per output row (B <= 65535; 8 x 512 ids in front of a ~30 ms step: not a throughput kernel).  A thread owns four
// consecutive tokens at a time.  Every stored row starts on a 16-byte boundary, so a quad that lies inside the row is ONE aligned 16-byte
// load (a row the caller placed elsewhere is read with single loads throughout); the quad that holds the row's end is peeled into single
// loads of the tokens that exist -- nothing past a row is ever read, and a
// src_row outside the store reads nothing at all.  The four int64 results leave as two 16-byte stores when their address allows (an ids
// row is 16-byte aligned only when ld_ids is even), else as single 8-byte stores; the quad that holds column L is peeled the same way:
// columns L .. ld_ids are never written.  No LDS, no atomics.
#include "common.h"
#include "srhip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(2))) long long i64x2_t;

__global__ __launch_bounds__(256) void token_view_kernel(const int* __restrict__ store, const long long* __restrict__ row_off,
                                                         const int* __restrict__ row_len, int n_rows, const long long* __restrict__ src_row,
                                                         int L, int pad_id, long long* __restrict__ ids, int ld_ids, int* __restrict__ key_len) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long r = src_row[b];
  int n = 0;                                          // tokens of the row that exist and fit; a row outside the store: none
  const int* p = store;
  if (r >= 0 && r < n_rows) {
    const int len = row_len[r];
    const long long off = row_off[r];
    if (len > 0 && off >= 0) {
      n = min(len, L);
      p = store + off;
    }
  }
  if (tid == 0) key_len[b] = n;
  const bool load16 = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  long long* __restrict__ o = ids + (size_t)b * ld_ids;
  const bool store16 = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
  for (int t0 = 4 * tid; t0 < L; t0 += 4 * 256) {
    i32x4_t v;
    if (load16 && t0 + 4 <= n) {
      v = *reinterpret_cast<const i32x4_t*>(p + t0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = t0 + j < n ? p[t0 + j] : pad_id;
    }
    if (store16 && t0 + 4 <= L) {
      i64x2_t lo, hi;
      lo[0] = v[0], lo[1] = v[1], hi[0] = v[2], hi[1] = v[3];
      *reinterpret_cast<i64x2_t*>(o + t0) = lo;
      *reinterpret_cast<i64x2_t*>(o + t0 + 2) = hi;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (t0 + j < L) o[t0 + j] = v[j];
    }
  }
}

}  // namespace

extern "C" int srhip_token_view(const int* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row, int B,
                                int L, int pad_id, long long* ids, int ld_ids, int* key_len, void* stream) {
  if (!store || !row_off || !row_len || !src_row || !ids || !key_len) return SR_EINVAL;
  if (n_rows <= 0 || B <= 0 || B > 65535 || L <= 0 || ld_ids < L) return SR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(store) & 15) || (reinterpret_cast<uintptr_t>(ids) & 7)) return SR_EINVAL;
  SR_LAUNCH(token_view_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, store, row_off, row_len, n_rows, src_row, L, pad_id, ids, ld_ids,
            key_len);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
