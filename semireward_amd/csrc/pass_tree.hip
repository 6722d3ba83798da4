// Pass-prefix sharing of the ViT inference rows (share_pass_prefixes): row-group copies between the nodes of a pass-prefix tree.
//
// The K + 1 passes of a SemiReward step forward the same images; two passes of one image differ only by their DropPath draws and stay
// bit-identical up to the first block where those differ.  The engine then computes each (image, draws so far) once: a node's rows are
// copied to its new children in front of the block where they split (fork), and after the last block every (pass, image) column takes
// the logits / feature of its node (fan-out).  Both are pure copies: the results stay those of the unshared launch, bit for bit.
//
// One kernel serves both: group g copies `bytes` bytes of each of (up to) two planes from group src[g] to group dst[g] (or dst0 + g),
// groups being equal-size contiguous slabs (an image's [N, D] rows, or one row of a [rows, C] table).  Per plane: 16-byte accesses when its
// slab and bases are 16-byte aligned (the [N, D] slabs of D = 128 / 384 / 768 always are), 4-byte ones otherwise (a [*, 10] logits table).
#include "common.h"
#include "srhip.h"

namespace {

struct CopyPlane {
  const char* src;
  char* dst;
  long long bytes;          // per group (0: plane unused)
  int v16;                  // 16-byte accesses (slab size and both bases 16-byte aligned), else 4-byte ones
};

template <typename V>
__device__ __forceinline__ void copy_slab(const CopyPlane& p, long long s, long long d) {
  const long long nv = p.bytes / (long long)sizeof(V);
  const V* __restrict__ sp = reinterpret_cast<const V*>(p.src + s * p.bytes);
  V* __restrict__ dp = reinterpret_cast<V*>(p.dst + d * p.bytes);
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += step) dp[i] = sp[i];
}

__global__ __launch_bounds__(256) void row_group_copy_kernel(CopyPlane p0, CopyPlane p1, const int* __restrict__ src_idx,
                                                             const long long* __restrict__ dst_idx, int dst0, int n, int src_groups,
                                                             long long dst_groups) {
  const int g = blockIdx.y;
  if (g >= n) return;
  const long long s = src_idx[g];
  const long long d = dst_idx ? dst_idx[g] : (long long)dst0 + g;
  if (s < 0 || s >= src_groups || d < 0 || d >= dst_groups) return;        // (the host validates the tables; a bad entry copies nothing)
  // the access width is chosen per plane (uniform over the launch: no divergence): a [*, 10] logits plane does not narrow the feature plane
  if (p0.v16) copy_slab<uint4>(p0, s, d); else copy_slab<uint32_t>(p0, s, d);
  if (p1.bytes) { if (p1.v16) copy_slab<uint4>(p1, s, d); else copy_slab<uint32_t>(p1, s, d); }
}

int launch_copy(CopyPlane p0, CopyPlane p1, const int* src_idx, const long long* dst_idx, int dst0, int n, int src_groups, long long dst_groups,
                hipStream_t s) {
  if (n <= 0) return SR_OK;
  if (!src_idx || n > 65535 || src_groups <= 0 || dst_groups <= 0 || p0.bytes <= 0 || p1.bytes < 0) return SR_EINVAL;
  if (!p0.src || !p0.dst || (p1.bytes && (!p1.src || !p1.dst))) return SR_EINVAL;
  if ((p0.bytes | p1.bytes) & 3) return SR_EINVAL;
  for (CopyPlane* p : {&p0, &p1}) p->v16 = !(p->bytes & 15) && !(((uintptr_t)p->src | (uintptr_t)p->dst) & 15);
  const long long most = max(p0.bytes / (p0.v16 ? 16 : 4), p1.bytes / (p1.v16 ? 16 : 4));
  const dim3 grid(min(cdiv(most, 256), 128), n);
  SR_LAUNCH(row_group_copy_kernel, grid, dim3(256), 0, s, p0, p1, src_idx, dst_idx, dst0, n, src_groups, dst_groups);
  SR_CHECK_LAUNCH();
  return SR_OK;
}

}  // namespace

extern "C" int srhip_vit_fork(float* x, void* ln, const int* parent, int n_new, int dst0, int rows_per_node, int D, void* stream) {
  if (!x || rows_per_node <= 0 || D <= 0 || dst0 <= 0) return SR_EINVAL;
  const long long slab = (long long)rows_per_node * D;
  CopyPlane px{reinterpret_cast<const char*>(x), reinterpret_cast<char*>(x), slab * 4, 0};
  CopyPlane pl{reinterpret_cast<const char*>(ln), reinterpret_cast<char*>(ln), ln ? slab * 2 : 0, 0};
  return launch_copy(px, pl, parent, nullptr, dst0, n_new, dst0, (long long)dst0 + n_new, (hipStream_t)stream);
}

extern "C" int srhip_vit_fanout(const float* node_logits, const float* node_feat, int n_nodes, const int* col_node, const long long* col_rows,
                                int n_cols, float* logits_all, float* feat_all, long long rows_all, int C, int D, void* stream) {
  if (!node_logits || !node_feat || !col_rows || !logits_all || !feat_all || n_nodes <= 0 || C <= 0 || D <= 0 || rows_all <= 0) return SR_EINVAL;
  CopyPlane pf{reinterpret_cast<const char*>(node_feat), reinterpret_cast<char*>(feat_all), (long long)D * 4, 0};
  CopyPlane pg{reinterpret_cast<const char*>(node_logits), reinterpret_cast<char*>(logits_all), (long long)C * 4, 0};
  return launch_copy(pf, pg, col_node, col_rows, 0, n_cols, n_nodes, rows_all, (hipStream_t)stream);
}
