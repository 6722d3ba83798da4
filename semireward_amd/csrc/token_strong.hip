// The strong view of a batch of token sequences made on the device from the CLEAN sentence of the resident token store
// (data/device_tokens.py, ``device_tokens_strong: True``): gather the row, apply two token-level slots (delete / mask / cutoff / swap, each
// with its own count and seed), truncate to L, right-pad with pad_id, widen int32 -> int64 and write the lengths -- one launch per view.
// The chain is the engine's own (it is NOT the reference's back-translation, which a translation model produced offline); its exact integer
// restatement is tests/_token_strong_cases.py (strong_row_ref) and the contract is in include/srhip.h.
//
// One 256-thread workgroup per output row.  The row is loaded into LDS as srhip_token_view reads it (aligned 16-byte loads inside the row, the
// quad that holds the row's end peeled: nothing past a row is read).  LDS holds two arrays of Lsrc ints: the row, and a second one that is the
// keys of a ranked selection while they are needed and the destination of a compaction afterwards (the two then change roles).  Per slot:
//   DELETE / MASK  key_i = fmix32(seed + i * 0x9E3779B1) of every interior position -> barrier -> every thread ranks the positions it owns by
//                  counting the smaller keys (16-byte LDS reads, all lanes the same address: a broadcast) -> barrier;  selected iff rank < c
//   CUTOFF         selected iff start <= i < start + c
//   MASK           the selected tokens become mask_id, in place
//   DELETE/CUTOFF  a thread owns ceil(n / 256) CONSECUTIVE positions: its survivors are counted, a block exclusive scan (Hillis-Steele over the
//                  256 counts, two LDS buffers) places them, and they are written in order into the other array
//   SWAP           every thread hashes: the c position pairs wait in the second array -> barrier -> one lane runs the exchanges in order
// with a barrier behind every phase.  op, c, seed and the row's length are made wave-uniform (readfirstlane) so that every barrier is reached
// under scalar control flow.  The row leaves like a srhip_token_view row: 16-byte stores where the address allows, the quad that holds column
// L peeled, columns L .. ld_ids never written.  No atomics: equal inputs give equal bits.
#include "common.h"
#include "srhip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4_t;
typedef __attribute__((ext_vector_type(2))) long long i64x2_t;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4_t;

constexpr uint32_t kGolden = 0x9E3779B1u;
constexpr int kThreads = 256;

struct Row {
  int* tok;        // the row as it stands
  int* alt;        // keys of a ranked selection, then the destination of a compaction
  int n;
};

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// One slot on the row in LDS.  Every thread of the workgroup calls it with the same (op, c, seed); ends behind a barrier.
__device__ __forceinline__ void apply_slot(Row& row, int op, int c, uint32_t seed, int mask_id, int* scan, int tid) {
  const int n = row.n, ni = max(0, n - 2);
  c = min(c, ni);
  if (op < SR_TOKEN_DELETE || op > SR_TOKEN_SWAP || c == 0) return;        // COPY, an unknown op, nothing to select: the row stays
  int* tok = row.tok;                                                        // (no __restrict__: the keys live in ``alt``)
  int* alt = row.alt;
  if (op == SR_TOKEN_SWAP) {
    if (ni >= 2) {                                                           // every thread hashes: the pairs (a | b << 16, both < 4096) wait in ``alt``
      for (int k = tid; k < c; k += kThreads) {
        const int a = 1 + (int)(fmix32(seed + (uint32_t)(2 * k) * kGolden) % (uint32_t)ni);
        const int b = 1 + (int)(fmix32(seed + (uint32_t)(2 * k + 1) * kGolden) % (uint32_t)ni);
        alt[k] = a | b << 16;
      }
      __syncthreads();
      if (tid == 0) {                                                        // one lane exchanges, in order of k
        int ab = alt[0];
        for (int k = 0; k < c; ++k) {
          const int a = ab & 0xffff, b = ab >> 16;
          ab = alt[min(k + 1, c - 1)];                                       // (the next pair is on its way while this one is exchanged)
          const int ta = tok[a], tb = tok[b];
          tok[a] = tb, tok[b] = ta;
        }
      }
    }
    __syncthreads();
    return;
  }
  const int per = (n + kThreads - 1) / kThreads;                             // <= 16: consecutive positions a thread owns
  const int lo = min(n, tid * per), hi = min(n, lo + per);
  uint32_t sel = 0;                                                          // bit k: position lo + k is selected
  if (op == SR_TOKEN_CUTOFF) {
    const int start = 1 + (int)(fmix32(seed) % (uint32_t)(ni - c + 1));
    for (int i = lo; i < hi; ++i)
      if (i >= start && i < start + c) sel |= 1u << (i - lo);
  } else {
    uint32_t* key = reinterpret_cast<uint32_t*>(alt);
    const int n4 = (n + 3) & ~3;                                             // <= Lq; outside the interior a key is 2^32 - 1: never below another
    for (int i = tid; i < n4; i += kThreads) key[i] = i >= 1 && i <= n - 2 ? fmix32(seed + (uint32_t)i * kGolden) : 0xFFFFFFFFu;
    __syncthreads();
    for (int i = max(lo, 1); i < min(hi, n - 1); ++i) {
      const uint32_t ki = key[i];
      int rank = 0;
#pragma unroll 8
      for (int j = 0; j < n4; j += 4) {                                      // 16-byte LDS reads, every lane the same address (a broadcast), eight in flight
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(key + j);
        rank += (v[0] < ki ? 1 : 0) + (v[1] < ki ? 1 : 0) + (v[2] < ki ? 1 : 0) + (v[3] < ki ? 1 : 0);
      }
      if (rank < c) sel |= 1u << (i - lo);
    }
    __syncthreads();                                                         // the keys are dead: ``alt`` may be written
  }
  if (op == SR_TOKEN_MASK) {
    for (int i = lo; i < hi; ++i)
      if (sel >> (i - lo) & 1u) tok[i] = mask_id;
    __syncthreads();
    return;
  }
  const int cnt = (hi - lo) - __popc(sel);
  scan[tid] = cnt;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < kThreads; d <<= 1) {                                   // inclusive scan, 8 rounds: the result is back in buffer 0
    const int v = scan[cur * kThreads + tid] + (tid >= d ? scan[cur * kThreads + tid - d] : 0);
    scan[(cur ^ 1) * kThreads + tid] = v;
    __syncthreads();
    cur ^= 1;
  }
  int dst = scan[cur * kThreads + tid] - cnt;
  for (int i = lo; i < hi; ++i)
    if (!(sel >> (i - lo) & 1u)) alt[dst++] = tok[i];
  __syncthreads();
  row.tok = alt, row.alt = tok, row.n = n - c;
}

__global__ __launch_bounds__(kThreads) void token_strong_kernel(const int* __restrict__ store, const long long* __restrict__ row_off,
                                                                const int* __restrict__ row_len, int n_rows,
                                                                const long long* __restrict__ src_row, const long long* __restrict__ slot0,
                                                                const long long* __restrict__ slot1, int Lsrc, int L, int pad_id, int mask_id,
                                                                long long* __restrict__ ids, int ld_ids, int* __restrict__ key_len) {
  extern __shared__ __attribute__((aligned(16))) int lds[];                  // two arrays of Lq ints
  __shared__ int scan[2 * kThreads];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int Lq = (Lsrc + 3) & ~3;
  const long long r = src_row[b];
  int n = 0;                                          // tokens of the row that exist and are taken; a row outside the store: none
  const int* p = store;
  if (r >= 0 && r < n_rows) {
    const int len = row_len[r];
    const long long off = row_off[r];
    if (len > 0 && off >= 0) {
      n = min(len, Lsrc);
      p = store + off;
    }
  }
  n = uniform(n);
  Row row = {lds, lds + Lq, n};
  const bool load16 = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
  for (int t0 = 4 * tid; t0 < n; t0 += 4 * kThreads) {
    if (load16 && t0 + 4 <= n) {
      *reinterpret_cast<i32x4_t*>(row.tok + t0) = *reinterpret_cast<const i32x4_t*>(p + t0);
    } else {
      for (int j = 0; j < 4 && t0 + j < n; ++j) row.tok[t0 + j] = p[t0 + j];
    }
  }
  __syncthreads();
  const unsigned long long s0 = (unsigned long long)slot0[b], s1 = (unsigned long long)slot1[b];
  apply_slot(row, uniform((int)(s0 & 0xffu)), uniform((int)((s0 >> 8) & 0xffffffu)), (uint32_t)uniform((int)(s0 >> 32)), mask_id, scan, tid);
  apply_slot(row, uniform((int)(s1 & 0xffu)), uniform((int)((s1 >> 8) & 0xffffffu)), (uint32_t)uniform((int)(s1 >> 32)), mask_id, scan, tid);
  const int m = min(row.n, L);                        // a row that would pass L is truncated, key_len with it
  if (tid == 0) key_len[b] = m;
  const int* __restrict__ tok = row.tok;
  long long* __restrict__ o = ids + (size_t)b * ld_ids;
  const bool store16 = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
  for (int t0 = 4 * tid; t0 < L; t0 += 4 * kThreads) {
    i32x4_t v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = t0 + j < m ? tok[t0 + j] : pad_id;
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

extern "C" int srhip_token_strong(const int* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row,
                                  const long long* slot0, const long long* slot1, int B, int Lsrc, int L, int pad_id, int mask_id,
                                  long long* ids, int ld_ids, int* key_len, void* stream) {
  if (!store || !row_off || !row_len || !src_row || !slot0 || !slot1 || !ids || !key_len) return SR_EINVAL;
  if (n_rows <= 0 || B <= 0 || B > 65535 || Lsrc <= 0 || Lsrc > SR_TOKEN_STRONG_MAX_LSRC || L <= 0 || ld_ids < L) return SR_EINVAL;
  if (pad_id < 0 || mask_id < 0) return SR_EINVAL;
  if ((reinterpret_cast<uintptr_t>(store) & 15) || (reinterpret_cast<uintptr_t>(ids) & 7)) return SR_EINVAL;
  const size_t lds_bytes = 2 * (size_t)((Lsrc + 3) & ~3) * sizeof(int);      // 32 KiB at the cap
  SR_LAUNCH(token_strong_kernel, dim3(B), dim3(kThreads), lds_bytes, (hipStream_t)stream, store, row_off, row_len, n_rows, src_row, slot0, slot1,
            Lsrc, L, pad_id, mask_id, ids, ld_ids, key_len);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
