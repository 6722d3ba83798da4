// Scoring a whole unlabelled set (AlgorithmBase.score_unlabeled, semireward_amd/core/pl_table.py): what the model, the algorithm's threshold
// rule and the Rewarder say about every row, WITHOUT touching any training state.  Two launches per batch around the Rewarder's forward:
//   srhip_score_rows     logits [B, C] -> per row: label, conf, margin, entropy and the threshold rule's mask / weight from the state AS IT STANDS
//   srhip_score_commit   the batch's dense columns + reward + reward filter -> the device tables of the whole set, at idx[b] or row_offset + b
// include/srhip.h holds the contract.  Reference lines of the four rules: masking.py:42-57, srflexmatch/utils.py:50-56,
// freematch/utils.py:24-66, srsoftmatch/utils.py:32-76 (+ hooks/dist_align.py:26-56).
//
// score_rows: one wave per row, four rows per workgroup.  (label, conf) must be the bits srhip_row_max gives, so the lanes own the columns
// in ITS layout (lane l: columns l, l + 64, ...) and the softmax body is the shared one of row_softmax.h.  That layout is not the one a
// 16-byte load delivers (four consecutive columns per lane), so a row travels global -> LDS -> registers: each wave stages up to 1024
// columns of its row in LDS with aligned 16-byte loads (the head up to the first 16-byte boundary and the tail peeled into scalar loads;
// every fp32 row start allows it), then reads its 16 columns per lane back in the row_max layout.  A row of C <= 1024 (the length eval.hip
// keeps in registers) is staged once and lives in registers through every sweep; longer rows are staged again, 1024 columns at a time,
// for every sweep (they hit L2).  Reductions are the xor butterflies of score_filter.hip (common.h wave_sum / wave_max, wave_argmax).
// expf / logf are the accurate library ones.  No atomics at all here: a launch on equal inputs gives equal bits.
//
// Rows beyond B in the last workgroup recompute row B - 1 and store nothing: every wave reaches every workgroup barrier.
#include "common.h"
#include "row_softmax.h"
#include "srhip.h"

#pragma clang fp contract(off)

namespace {

constexpr int ROWS = 4;                   // waves (rows) per workgroup
constexpr int CHUNK = 1024;               // columns staged at a time: 16 per lane
constexpr int KREG = CHUNK / 64;
constexpr int IDX_ERR_BIT = 64;           // bit 6 of the label-error word

struct ScoreArgs {
  const float* logits; long long ld;
  const float* acc;                       // FLEX
  const float* time_p; const float* p_model;          // FREE
  const float* mu_var;                    // SOFT
  const float* da_p_model; const float* da_p_target; const int* da_inited;     // SOFT + distribution alignment
  long long* label; float* conf; float* margin; float* entropy; float* weight;
  float p_cutoff;
  int n_sigma, mode, B, C;
};

// columns [cb, cend) of row z into st[a + (c - cb)], a = the row start's offset from a 16-byte boundary in elements: every aligned
// quad of the row is one 16-byte load and one 16-byte LDS store
__device__ __forceinline__ void stage_chunk(const float* __restrict__ z, float* __restrict__ st, int a, int cb, int cend, int lane) {
  const int head = (4 - a) & 3;           // columns in front of the first 16-byte boundary of the chunk (cb is a multiple of 4)
  if (lane < head && cb + lane < cend) st[a + lane] = z[cb + lane];
#pragma unroll
  for (int j = 0; j < KREG / 4; ++j) {                   // 256 quads from the boundary on reach the chunk's end whatever the head; the last may be partial
    const int c0 = cb + head + 4 * (lane + 64 * j);
    if (c0 + 4 <= cend) {
      *reinterpret_cast<f32x4_t*>(st + a + (c0 - cb)) = *reinterpret_cast<const f32x4_t*>(z + c0);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (c0 + i < cend) st[a + (c0 - cb) + i] = z[c0 + i];
    }
  }
}

template <bool CACHED> __global__ __launch_bounds__(ROWS * 64) void score_rows_kernel(ScoreArgs A) {
  __shared__ __attribute__((aligned(16))) float stage[ROWS][CHUNK + 8];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row_raw = blockIdx.x * ROWS + wave;
  const bool live = row_raw < A.B;
  const int row = live ? row_raw : A.B - 1;
  const int C = A.C;
  const float* z = A.logits + (size_t)row * A.ld;
  const int a = (int)(((uintptr_t)z >> 2) & 3u);
  float* st = stage[wave];

  float zr[KREG];
  if constexpr (CACHED) {
    stage_chunk(z, st, a, 0, C, lane);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KREG; ++k) zr[k] = lane + 64 * k < C ? st[a + lane + 64 * k] : 0.f;
  }
  // the calling lane's columns in ascending order (row_softmax.h); every wave of the workgroup runs the same number of sweeps
  auto sweep = [&](auto&& g) {
    if constexpr (CACHED) {
#pragma unroll
      for (int k = 0; k < KREG; ++k)
        if (lane + 64 * k < C) g(lane + 64 * k, zr[k]);
    } else {
      for (int cb = 0; cb < C; cb += CHUNK) {
        const int cend = min(cb + CHUNK, C);
        __syncthreads();                                 // the previous chunk has been read
        stage_chunk(z, st, a, cb, cend, lane);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < KREG; ++k)
          if (cb + lane + 64 * k < cend) g(cb + lane + 64 * k, st[a + lane + 64 * k]);
      }
    }
  };

  float mx, inv;
  row_softmax_norm(sweep, mx, inv);

  const bool align = A.mode == SRHIP_SCORE_SOFT && A.da_inited != nullptr && *A.da_inited != 0;
  float bv, b2 = 0.f, ent = 0.f;          // b2: the second largest probability (0 for C == 1: margin = conf)
  int bi;
  auto take = [&](int c, float p) {
    if (p > bv) { b2 = fmaxf(b2, bv); bv = p; bi = c; }
    else if (p > b2) b2 = p;              // an equal of the maximum lands here: margin 0 for a tie at the top
    if (p > 0.f) ent += p * logf(p);      // 0 ln 0 = 0
  };
  if (!align) {
    bv = -INFINITY; bi = 0x7fffffff;      // srhip_row_max's start values
    sweep([&](int c, float zc) { take(c, row_softmax_prob(zc, mx, inv)); });
  } else {
    // DistAlignEMAHook.dist_align (dist_align.py:31-32) as distalign_kernel forms it: p (pt + 1e-6) / (pm + 1e-6), renormalised by its row sum
    const float* pm = A.da_p_model;
    const float* pt = A.da_p_target;
    float s = 0.f;
    sweep([&](int c, float zc) { s += row_softmax_prob(zc, mx, inv) * (pt[c] + 1e-6f) / (pm[c] + 1e-6f); });
    s = wave_sum(s);
    bv = -1.0f; bi = 0;                   // distalign_kernel's start values
    sweep([&](int c, float zc) {
      const float al = row_softmax_prob(zc, mx, inv) * (pt[c] + 1e-6f) / (pm[c] + 1e-6f);
      take(c, al / s);
    });
  }
  // (value, column) butterfly of wave_argmax, carrying the runner-up: the two sides of a stage hold disjoint columns
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64), o2 = __shfl_xor(b2, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > bv || (ov == bv && oi < bi)) { b2 = fmaxf(bv, o2); bv = ov; bi = oi; }
    else b2 = fmaxf(b2, ov);
  }
  ent = wave_sum(ent);

  const float conf = bv;
  const bool in_range = (unsigned)bi < (unsigned)C;      // a row of NaNs has no argmax (srhip_row_max: 0x7fffffff): its weight is 0
  float w = 0.f;
  if (A.mode == SRHIP_SCORE_FIXED) {                     // masking.py:53
    w = conf >= A.p_cutoff ? 1.0f : 0.0f;
  } else if (A.mode == SRHIP_SCORE_FLEX) {               // srflexmatch/utils.py:53, the order of flexmatch_mask_lds_kernel
    if (in_range) {
      const float acc = A.acc[bi];
      const float den = 2.0f - acc;
      const float rat = acc / den;
      const float thr = A.p_cutoff * rat;
      w = conf >= thr ? 1.0f : 0.0f;
    }
  } else if (A.mode == SRHIP_SCORE_FREE) {               // freematch/utils.py:62-66, the order of freematch_update_kernel
    float pmax = 0.f;
    for (int c = lane; c < C; c += 64) pmax = fmaxf(pmax, A.p_model[c]);
    pmax = wave_max(pmax);
    if (in_range) {
      const float mod = A.p_model[bi] / pmax;
      w = conf >= A.time_p[0] * mod ? 1.0f : 0.0f;
    }
  } else {                                               // srsoftmatch/utils.py:68-75, the order of softmatch_mask_kernel
    const float mu = A.mu_var[0], den = (2.0f * A.mu_var[1]) / (float)(A.n_sigma * A.n_sigma);
    const float d = fminf(conf - mu, 0.0f);
    w = expf(-((d * d) / den));
  }
  if (live && lane == 0) {
    A.label[row] = bi;
    A.conf[row] = conf;
    A.margin[row] = conf - b2;
    A.entropy[row] = 0.f - ent;
    A.weight[row] = w;
  }
}

struct CommitArgs {
  const long long* label; const float* conf; const float* margin; const float* entropy; const float* weight;
  const float* reward; const float* keep;
  const long long* idx; long long row_offset, n;
  long long* t_label; float* t_conf; float* t_margin; float* t_entropy; float* t_weight; float* t_reward;
  unsigned char* t_keep; unsigned char* t_selected; int* t_count;
  int* label_err;
  int B;
};

__global__ __launch_bounds__(256) void score_commit_kernel(CommitArgs A) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= A.B) return;
  const long long j = A.idx ? A.idx[b] : A.row_offset + b;
  if (j < 0 || j >= A.n) {                // skipped: nothing is written out of bounds; the host raises at its next read of the word
    atomicOr(A.label_err, IDX_ERR_BIT);
    return;
  }
  const float w = A.weight[b];
  const bool keep = A.keep[b] > 0.f;
  A.t_label[j] = A.label[b];
  A.t_conf[j] = A.conf[b];
  A.t_margin[j] = A.margin[b];
  A.t_entropy[j] = A.entropy[b];
  A.t_weight[j] = w;
  A.t_reward[j] = A.reward[b];
  A.t_keep[j] = keep ? 1 : 0;
  A.t_selected[j] = (w > 0.f && keep) ? 1 : 0;
  atomicAdd(A.t_count + j, 1);
}

inline bool al8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

}  // namespace

extern "C" int srhip_score_rows(const float* logits, long long ld, int B, int C, int mode, float p_cutoff, const float* classwise_acc,
                                const float* time_p, const float* p_model, const float* mu_var, int n_sigma, const float* da_p_model,
                                const float* da_p_target, const int* da_inited, long long* label, float* conf, float* margin,
                                float* entropy, float* weight, void* stream) {
  if (!logits || !label || !conf || !margin || !entropy || !weight) return SR_EINVAL;
  if (B < 1 || B > 65535 || C < 1 || ld < C) return SR_EINVAL;
  if (!al8(label)) return SR_EINVAL;
  switch (mode) {
    case SRHIP_SCORE_FIXED: break;
    case SRHIP_SCORE_FLEX: if (!classwise_acc) return SR_EINVAL; break;
    case SRHIP_SCORE_FREE: if (!time_p || !p_model) return SR_EINVAL; break;
    case SRHIP_SCORE_SOFT:
      if (!mu_var || n_sigma <= 0) return SR_EINVAL;
      if ((da_p_model || da_p_target || da_inited) && !(da_p_model && da_p_target && da_inited)) return SR_EINVAL;    // all three or none
      break;
    default: return SR_EINVAL;
  }
  const ScoreArgs a{logits, ld, classwise_acc, time_p, p_model, mu_var, da_p_model, da_p_target, da_inited,
                    label, conf, margin, entropy, weight, p_cutoff, n_sigma, mode, B, C};
  if (C <= CHUNK) SR_LAUNCH((score_rows_kernel<true>), dim3(cdiv(B, ROWS)), dim3(ROWS * 64), 0, (hipStream_t)stream, a);
  else SR_LAUNCH((score_rows_kernel<false>), dim3(cdiv(B, ROWS)), dim3(ROWS * 64), 0, (hipStream_t)stream, a);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

extern "C" int srhip_score_commit(const long long* label, const float* conf, const float* margin, const float* entropy, const float* weight,
                                  const float* reward, const float* reward_keep, const long long* idx, long long row_offset, int B,
                                  long long n, long long* t_label, float* t_conf, float* t_margin, float* t_entropy, float* t_weight,
                                  float* t_reward, unsigned char* t_reward_keep, unsigned char* t_selected, int* t_count, void* stream) {
  if (!label || !conf || !margin || !entropy || !weight || !reward || !reward_keep) return SR_EINVAL;
  if (!t_label || !t_conf || !t_margin || !t_entropy || !t_weight || !t_reward || !t_reward_keep || !t_selected || !t_count) return SR_EINVAL;
  if (B < 1 || B > 65535 || n < 1 || (!idx && row_offset < 0)) return SR_EINVAL;
  if (!al8(label) || !al8(t_label) || (idx && !al8(idx))) return SR_EINVAL;
  int* err = sr_label_err_ptr();
  if (!err) return SR_ELAUNCH;
  const CommitArgs a{label, conf, margin, entropy, weight, reward, reward_keep, idx, row_offset, n, t_label, t_conf, t_margin, t_entropy,
                     t_weight, t_reward, t_reward_keep, t_selected, t_count, err, B};
  SR_LAUNCH(score_commit_kernel, dim3(cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, a);
  SR_CHECK_LAUNCH();
  return SR_OK;
}
