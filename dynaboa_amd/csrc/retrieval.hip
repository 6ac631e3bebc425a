// Device-resident exemplar retrieval (reference base_adaptor.py:82-96): the nearest cluster centre to a level's pooled feature by
// cosine distance, one member of that cluster drawn by a counter-based generator, and the chosen exemplar copied out of the resident
// bank into the stepper's exemplar inputs - what BaseAdaptor.retrieval does on the host (an `.item()`, a PNG decode, five uploads),
// without leaving the device.
//
// dyb_retrieve_select: two launches.  (1) One workgroup per (centre chunk, row): the row's 2048 floats sit in registers (8 float4 per
// lane, the same in each of the 4 waves), a wave takes the chunk's centres one at a time - eight 16-byte loads per lane, a 64-lane
// butterfly - and keeps its best (cos, k); the workgroup's best goes to the workspace.  cos_k = dot(x, c_k) * inv_norm_k: the row's own
// norm is a positive common factor.  A centre's dot product is summed in ONE fixed order (lane-serial over the eight float4, then the
// butterfly) whatever the chunking, and the maximum over (cos, -k) is exact, so the answer does not depend on the grid shape or on the
// order in which workgroups finish.  (2) One wave per row folds the chunk partials (ties to the LOWEST centre index), draws the
// member and writes (cluster, item) into the row's pick log.
// Rows are addressed by (physical replica index, byte stride) pairs given by the caller: the stepper passes its launch scope's replicas
// and the stride of its per-replica arenas, a caller with plain [n][...] tensors passes 0 .. n-1 and the row pitch.
#include <math.h>

#include "dyb_common.h"
#include "dyb_philox.h"

#define RETR_D 2048                 // pooled feature / centre length (features[5])
#define RETR_DEFAULT_CHUNK 16       // centres per workgroup (4 per wave)
#define RETR_MAX_ROWS DYB_MAX_REPLICAS

struct RetrRows {
  int n;
  int row[RETR_MAX_ROWS];                     // physical replica of launch row i
  unsigned long long draw[RETR_MAX_ROWS];     // its draw index (host state)
};
struct RetrPart {
  float cos;
  int k;
};
// (cos, -k) order: larger cosine wins, equal cosines go to the lower centre index.  NaN compares false both ways: it never wins.
__device__ __forceinline__ bool retr_better(float c, int k, float bc, int bk) { return c > bc || (c == bc && k < bk); }

__global__ __launch_bounds__(256) void retrieve_select_kernel(const float* __restrict__ feat, size_t feat_stride,
                                                              const float* __restrict__ centers, const float* __restrict__ inv_norm, int K,
                                                              int chunk, RetrPart* __restrict__ part, RetrRows rows) {
  __shared__ float s_cos[4];
  __shared__ int s_k[4];
  const int slot = blockIdx.y, ch = blockIdx.x, nch = gridDim.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float4* x4 = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(feat) + (size_t)rows.row[slot] * feat_stride);
  float4 x[RETR_D / 256];
#pragma unroll
  for (int j = 0; j < RETR_D / 256; ++j) x[j] = x4[j * 64 + lane];
  const int k0 = ch * chunk, k1 = (k0 + chunk < K) ? k0 + chunk : K;
  float best = -INFINITY;
  int bk = k0;
  for (int k = k0 + wave; k < k1; k += 4) {
    const float4* c4 = reinterpret_cast<const float4*>(centers + (size_t)k * RETR_D);
    float4 c[RETR_D / 256];
#pragma unroll
    for (int j = 0; j < RETR_D / 256; ++j) c[j] = c4[j * 64 + lane];
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < RETR_D / 256; ++j) {
      acc = fmaf(x[j].x, c[j].x, acc); acc = fmaf(x[j].y, c[j].y, acc);
      acc = fmaf(x[j].z, c[j].z, acc); acc = fmaf(x[j].w, c[j].w, acc);
    }
    const float cs = dyb_wave_sum(acc) * inv_norm[k];
    if (retr_better(cs, k, best, bk)) { best = cs; bk = k; }
  }
  if (lane == 0) { s_cos[wave] = best; s_k[wave] = bk; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w)
      if (retr_better(s_cos[w], s_k[w], best, bk)) { best = s_cos[w]; bk = s_k[w]; }
    part[(size_t)slot * nch + ch] = RetrPart{best, bk};
  }
}

// status[slot]: 0 = a pick was written; 1 = the nearest cluster is empty; 2 = the membership tables point outside the bank.  A row
// that fails gets item -1 in its pick log (dyb_exemplar_gather leaves such a replica's exemplar inputs untouched).
__global__ __launch_bounds__(64) void retrieve_resolve_kernel(const RetrPart* __restrict__ part, int nch, const int* __restrict__ member_ptr,
                                                              const int* __restrict__ member_idx, int n_members, int n_items,
                                                              unsigned seed_lo, unsigned seed_hi, unsigned sample, int* __restrict__ picks,
                                                              size_t picks_stride, int capacity, int* __restrict__ status, RetrRows rows) {
  const int slot = blockIdx.x, lane = threadIdx.x;
  float best = -INFINITY;
  int bk = 0x7fffffff;
  for (int c = lane; c < nch; c += 64) {
    const RetrPart p = part[(size_t)slot * nch + c];
    if (bk == 0x7fffffff || retr_better(p.cos, p.k, best, bk)) { best = p.cos; bk = p.k; }
  }
  for (int m = 32; m >= 1; m >>= 1) {
    const float oc = __shfl_xor(best, m);
    const int ok = __shfl_xor(bk, m);
    if (ok != 0x7fffffff && (bk == 0x7fffffff || retr_better(oc, ok, best, bk))) { best = oc; bk = ok; }
  }
  if (lane != 0) return;
  const int lo = member_ptr[bk], n = member_ptr[bk + 1] - lo;
  int item = -1, st = 0;
  const unsigned long long draw = rows.draw[slot];
  if (n <= 0) {
    st = 1;
  } else if (lo < 0 || lo + n > n_members) {
    st = 2;
  } else {
    unsigned w[4];
    philox4x32_10((unsigned)draw, (unsigned)(draw >> 32), sample, 0u, seed_lo, seed_hi, w);
    const int j = (int)(((unsigned long long)w[0] * (unsigned long long)(unsigned)n) >> 32);       // mulhi32(w, n): uniform in [0, n)
    item = member_idx[lo + j];
    if (item < 0 || item >= n_items) { item = -1; st = 2; }
  }
  int* row = reinterpret_cast<int*>(reinterpret_cast<char*>(picks) + (size_t)rows.row[slot] * picks_stride) + 2 * (size_t)(draw % (unsigned long long)capacity);
  row[0] = bk;
  row[1] = item;
  status[slot] = st;
}

static size_t retr_status_bytes() { return RETR_MAX_ROWS * sizeof(int); }
static int retr_chunk(int chunk) { return chunk > 0 ? chunk : RETR_DEFAULT_CHUNK; }
// workspace of dyb_retrieve_select for up to `rows` rows over K centres in chunks of `chunk` (<= 0: the default)
extern "C" size_t dyb_retrieve_workspace_bytes(int rows, int K, int chunk) {
  if (rows <= 0 || K <= 0) return 0;
  return retr_status_bytes() + (size_t)rows * dyb_cdiv(K, retr_chunk(chunk)) * sizeof(RetrPart);
}
static int retr_rows(const int* rows, int nrows, const unsigned long long* draws, RetrRows* out) {
  DYB_REQUIRE(rows && draws && nrows >= 1 && nrows <= RETR_MAX_ROWS, DYB_ERR_ARG);
  out->n = nrows;
  for (int i = 0; i < nrows; ++i) {
    DYB_REQUIRE(rows[i] >= 0 && rows[i] < RETR_MAX_ROWS, DYB_ERR_ARG);
    out->row[i] = rows[i];
    out->draw[i] = draws[rows[i]];
  }
  return DYB_OK;
}
// feat: row r at feat + rows[i] * feat_stride bytes (16-byte aligned); centers [K][2048]; center_inv_norm [K]; member_ptr [K + 1] /
// member_idx [n_members]: the clusters' members as CSR, item indices < n_items; rows / draws: HOST arrays - the physical replica of each
// of the nrows rows, and the draw index of every physical replica (indexed by replica, not by row); picks: replica r's log at picks +
// r * picks_stride bytes, [pick_capacity][2] int32, row draw mod pick_capacity = (cluster, item).  check != 0: the call waits for the
// stream and returns DYB_ERR_ARG if a row's nearest cluster is empty (or the tables point outside the bank) - the one synchronising
// form, for callers that read the picks next anyway; check == 0 never synchronises and such a row's item is -1.
extern "C" int dyb_retrieve_select(const float* feat, size_t feat_stride, const int* rows, int nrows, const float* centers,
                                   const float* center_inv_norm, int K, const int* member_ptr, const int* member_idx, int n_members,
                                   int n_items, const unsigned long long* draws, unsigned long long seed, int sample, int* picks,
                                   size_t picks_stride, int pick_capacity, int chunk, int check, void* ws, size_t ws_bytes,
                                   hipStream_t st) {
  DYB_REQUIRE(feat && centers && center_inv_norm && member_ptr && member_idx && picks && ws, DYB_ERR_ARG);
  DYB_REQUIRE(K > 0 && n_members > 0 && n_items > 0 && pick_capacity > 0 && sample >= 0, DYB_ERR_ARG);
  DYB_REQUIRE(((uintptr_t)feat & 15) == 0 && (feat_stride & 15) == 0 && ((uintptr_t)centers & 15) == 0, DYB_ERR_ARG);
  DYB_REQUIRE(((uintptr_t)picks & 3) == 0 && (picks_stride & 3) == 0 && ((uintptr_t)ws & 7) == 0, DYB_ERR_ARG);
  RetrRows R;
  {
    const int rc = retr_rows(rows, nrows, draws, &R);
    if (rc != DYB_OK) return rc;
  }
  chunk = retr_chunk(chunk);
  const int nch = dyb_cdiv(K, chunk);
  DYB_REQUIRE(ws_bytes >= dyb_retrieve_workspace_bytes(nrows, K, chunk), DYB_ERR_WORKSPACE);
  int* status = reinterpret_cast<int*>(ws);
  RetrPart* part = reinterpret_cast<RetrPart*>(reinterpret_cast<char*>(ws) + retr_status_bytes());
  hipLaunchKernelGGL(retrieve_select_kernel, dim3(nch, nrows, 1), dim3(256), 0, st, feat, feat_stride, centers, center_inv_norm, K, chunk,
                     part, R);
  DYB_CHECK_LAUNCH();
  hipLaunchKernelGGL(retrieve_resolve_kernel, dim3(nrows, 1, 1), dim3(64), 0, st, (const RetrPart*)part, nch, member_ptr, member_idx,
                     n_members, n_items, (unsigned)seed, (unsigned)(seed >> 32), (unsigned)sample, picks, picks_stride, pick_capacity,
                     status, R);
  DYB_CHECK_LAUNCH();
  if (check) {
    int host[RETR_MAX_ROWS];
    if (hipMemcpyAsync(host, status, (size_t)nrows * sizeof(int), hipMemcpyDeviceToHost, st) != hipSuccess) return DYB_ERR_LAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return DYB_ERR_LAUNCH;
    for (int i = 0; i < nrows; ++i) DYB_REQUIRE(host[i] == 0, DYB_ERR_ARG);
  }
  return DYB_OK;
}

// ---- gather: item picks[r][draw mod capacity][1] of the bank -> the five exemplar inputs of replica r ---------------------------------
#define EX_IMG_F4 (3 * 224 * 224 / 4)         // 37632 float4 per image
#define EX_KP 147
#define EX_POSE 72
#define EX_BETAS 10
#define EX_POSE3D 96
struct GatherDst {
  float* p[5];
  size_t stride[5];                           // bytes between consecutive replicas
};
__global__ __launch_bounds__(256) void exemplar_gather_kernel(const int* __restrict__ picks, size_t picks_stride, int capacity,
                                                              const float* __restrict__ img, const float* __restrict__ kp,
                                                              const float* __restrict__ pose, const float* __restrict__ betas,
                                                              const float* __restrict__ pose3d, int n_items, GatherDst d, RetrRows rows) {
  const int slot = blockIdx.y, r = rows.row[slot], t = threadIdx.x;
  const int* row = reinterpret_cast<const int*>(reinterpret_cast<const char*>(picks) + (size_t)r * picks_stride) +
                   2 * (size_t)(rows.draw[slot] % (unsigned long long)capacity);
  const int item = row[1];
  if (item < 0 || item >= n_items) return;                 // a failed pick: the replica's inputs stay as they are
  auto dst = [&](int k) { return reinterpret_cast<float*>(reinterpret_cast<char*>(d.p[k]) + (size_t)r * d.stride[k]); };
  const int nb = gridDim.x - 1;                            // image workgroups; the last workgroup copies the four small tables
  if ((int)blockIdx.x < nb) {
    const float4* s = reinterpret_cast<const float4*>(img) + (size_t)item * EX_IMG_F4;
    float4* o = reinterpret_cast<float4*>(dst(0));
    for (int i = blockIdx.x * 256 + t; i < EX_IMG_F4; i += nb * 256) o[i] = s[i];
    return;
  }
  // (rows of 147 / 10 floats are not 16-byte aligned in the bank: float by float, 325 floats in all)
  float* o1 = dst(1); float* o2 = dst(2); float* o3 = dst(3); float* o4 = dst(4);
  for (int i = t; i < EX_KP; i += 256) o1[i] = kp[(size_t)item * EX_KP + i];
  for (int i = t; i < EX_POSE; i += 256) o2[i] = pose[(size_t)item * EX_POSE + i];
  for (int i = t; i < EX_BETAS; i += 256) o3[i] = betas[(size_t)item * EX_BETAS + i];
  for (int i = t; i < EX_POSE3D; i += 256) o4[i] = pose3d[(size_t)item * EX_POSE3D + i];
}
// bank: img [n_items][3][224][224], kp [n_items][49][3], pose [n_items][72], betas [n_items][10], pose3d [n_items][24][4], fp32;
// dst5 / dst_stride5: HOST arrays - replica 0's five destinations (img 16-byte aligned) and the bytes between consecutive replicas of
// each; rows / draws / picks as in dyb_retrieve_select (the pick read is row draws[r] mod pick_capacity of replica r's log).
extern "C" int dyb_exemplar_gather(const int* picks, size_t picks_stride, int pick_capacity, const int* rows, int nrows,
                                   const unsigned long long* draws, const float* img, const float* kp, const float* pose,
                                   const float* betas, const float* pose3d, int n_items, float* const* dst5, const size_t* dst_stride5,
                                   hipStream_t st) {
  DYB_REQUIRE(picks && img && kp && pose && betas && pose3d && dst5 && dst_stride5 && n_items > 0 && pick_capacity > 0, DYB_ERR_ARG);
  DYB_REQUIRE(((uintptr_t)picks & 3) == 0 && (picks_stride & 3) == 0 && ((uintptr_t)img & 15) == 0, DYB_ERR_ARG);
  RetrRows R;
  {
    const int rc = retr_rows(rows, nrows, draws, &R);
    if (rc != DYB_OK) return rc;
  }
  GatherDst d;
  for (int k = 0; k < 5; ++k) {
    DYB_REQUIRE(dst5[k] && (dst_stride5[k] & 3) == 0, DYB_ERR_ARG);
    d.p[k] = dst5[k];
    d.stride[k] = dst_stride5[k];
  }
  DYB_REQUIRE(((uintptr_t)d.p[0] & 15) == 0 && (d.stride[0] & 15) == 0, DYB_ERR_ARG);
  hipLaunchKernelGGL(exemplar_gather_kernel, dim3(37, nrows, 1), dim3(256), 0, st, picks, picks_stride, pick_capacity, img, kp, pose, betas,
                     pose3d, n_items, d, R);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
