// The views of one step joined into one token batch (nets/bert.py, TokenBatch.cat with unequal padded lengths; ``token_len_bucket``): up to
// four right-padded id blocks of different widths become one [sum S, L_out] block, every row filled up with pad_id, and the two length
// vectors the engine carries beside it -- one launch.
//
// Replaces, per step: torch.zeros of the joined block, one slice copy per view, one torch.full per view for seq_len and the two torch.cat
// of the length vectors (about ten launches and three allocations in front of the step's first GEMM).
//
// One 256-thread workgroup per output row (sum S <= 65535; 24 x 512 ids in front of a ~30 ms step: not a throughput kernel).  The sources
// ride in the kernel's arguments, the workgroup finds its source by walking the at most four row counts.  A thread owns two consecutive
// ids (16 bytes) at a time.  A pair that lies inside the source row is ONE 16-byte load and a pair that lies inside the output row ONE
// 16-byte store when BOTH row addresses are 16-byte aligned (a source row is when its block is and L is even, an output row when L_out is
// even), else two 8-byte accesses; the pair that holds the source row's end is peeled into single loads of the ids that exist, the pair
// that holds column L_out into the single store that exists -- nothing past a source row is read, nothing past an output row written.
// No LDS, no atomics.
#include "common.h"
#include "srhip.h"

namespace {

typedef __attribute__((ext_vector_type(2))) long long i64x2_t;

struct token_cat_args {
  srhip_token_src src[SR_TOKEN_CAT_MAX_SRC];
  int n_src;
};

__global__ __launch_bounds__(256) void token_cat_kernel(token_cat_args a, int pad_id, long long* __restrict__ ids, int L_out,
                                                        int* __restrict__ key_len, int* __restrict__ seq_len) {
  const int b = blockIdx.x, tid = threadIdx.x;
  int j = 0, r = b;                                   // source j, its row r (the host sized the grid to sum S: the walk ends inside)
  while (j + 1 < a.n_src && r >= a.src[j].S) r -= a.src[j++].S;
  const srhip_token_src s = a.src[j];
  const int L = s.L;
  const long long* __restrict__ p = s.ids + (size_t)r * L;
  long long* __restrict__ o = ids + (size_t)b * L_out;
  if (tid == 0) {
    key_len[b] = s.key_len[r];
    seq_len[b] = s.seq_len ? s.seq_len[r] : L;
  }
  const bool wide = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(o)) & 15) == 0;
  const long long pad = pad_id;
  for (int t0 = 2 * tid; t0 < L_out; t0 += 2 * 256) {
    i64x2_t v;
    if (wide && t0 + 2 <= L) {
      v = *reinterpret_cast<const i64x2_t*>(p + t0);
    } else {
      v[0] = t0 < L ? p[t0] : pad;
      v[1] = t0 + 1 < L ? p[t0 + 1] : pad;
    }
    if (wide && t0 + 2 <= L_out) {
      *reinterpret_cast<i64x2_t*>(o + t0) = v;
    } else {
      o[t0] = v[0];
      if (t0 + 1 < L_out) o[t0 + 1] = v[1];
    }
  }
}

}  // namespace

extern "C" int srhip_token_cat(const srhip_token_src* src, int n_src, int pad_id, long long* ids, int L_out, int* key_len, int* seq_len,
                               void* stream) {
  if (!src || !ids || !key_len || !seq_len || n_src < 1 || n_src > SR_TOKEN_CAT_MAX_SRC || L_out <= 0 || pad_id < 0) return SR_EINVAL;
  if (reinterpret_cast<uintptr_t>(ids) & 7) return SR_EINVAL;
  token_cat_args a = {};
  long long rows = 0;
  for (int j = 0; j < n_src; ++j) {
    const srhip_token_src& s = src[j];
    if (!s.ids || !s.key_len || s.S <= 0 || s.L <= 0 || s.L > L_out || (reinterpret_cast<uintptr_t>(s.ids) & 7)) return SR_EINVAL;
    a.src[j] = s;
    rows += s.S;
  }
  if (rows > 65535) return SR_EINVAL;
  a.n_src = n_src;
  SR_LAUNCH(token_cat_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a, pad_id, ids, L_out, key_len, seq_len);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
