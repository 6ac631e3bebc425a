// Spherical k-means over a feature matrix, for building the exemplar retrieval index (dynaboa_amd/retrieval_index.py): the three
// device steps of one Lloyd iteration.  x is [N][D] fp32 with a row pitch in bytes, centres are [K][D] contiguous and stay
// un-normalised (every consumer divides by the norm), cosines are (dot(x_i, c_k) * inv|x_i|) * inv|c_k| with both inverse norms
// clamped as torch.cosine_similarity clamps them (1 / max(|v|, 1e-8)).
//
// dyb_rows_inv_norm   one wave per row: the squares summed lane-serially over the row's float4s, then the 64-lane butterfly.
// dyb_kmeans_assign   an [N][D] x [D][K] product on the exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32) with an argmax epilogue:
//                     a workgroup owns 128 rows (32 per wave) and walks the centres in passes of NT column tiles of 32 (NT = 1, 2 or 4,
//                     by K), D in steps of 32 through two LDS stages.  Both operand tiles lie ROW-major in LDS with a pitch of 36
//                     floats: a lane of half h reads the 16 consecutive k = 16h .. 16h + 15 of its row with four conflict-free
//                     16-byte reads and feeds them to 16 MFMAs - which k meets which inside an MFMA does not matter as long as A and
//                     B agree.  A running (best, index) per row is carried across the passes, so no score reaches memory.  Order
//                     (cos, -k): ties go to the LOWEST centre, the rule of dyb_retrieve_select.  A centre's dot product is summed
//                     in one fixed order whatever N, K or the grid, so assign / best do not depend on the tiling.
// dyb_kmeans_update   centre k = mean of x_i * inv|x_i| over its members, with NO floating-point atomics: rows are cut into chunks of
//                     R = R(N, K) rows; a workgroup (row chunk, 256 columns, 16 or 32 clusters) adds its chunk's member rows in
//                     ascending order into an LDS table [clusters][256], a thread per column, and writes the table to the workspace;
//                     a second launch adds the chunk partials in a fixed tree and divides by counts[k].  The summation order is a function
//                     of (N, D, K) alone: two calls return equal bytes.  counts[k] == 0 leaves centre k untouched.
#include <math.h>

#include "dyb_common.h"

#define KM_ROWS 128                // rows per assign workgroup
#define KM_STEP 32                 // floats of D per LDS stage
#define KM_LD 36                   // LDS pitch in floats: 16-byte reads of 32 consecutive rows at one k offset touch every bank once
#define KM_MAX_K 1024
#define KM_UP_UNROLL 8             // rows a thread of the update has in flight
#define KM_UP_COLS 256             // columns per update workgroup
#define KM_UP_BLOCK 2048           // rows listed at a time by the update of K > 32 (8 per thread)

__device__ __forceinline__ bool km_better(float c, int k, float bc, int bk) { return c > bc || (c == bc && k < bk); }

__global__ __launch_bounds__(256) void rows_inv_norm_kernel(const float* __restrict__ x, size_t x_stride, int N, int D,
                                                            float* __restrict__ inv_norm) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long want = (long long)blockIdx.x * 4 + wave;
  const long long row = want < N ? want : N - 1;                       // (a wave past the end repeats the last row and writes nothing)
  const float4* x4 = reinterpret_cast<const float4*>(reinterpret_cast<const char*>(x) + (size_t)row * x_stride);
  float acc = 0.f;
  for (int c = lane; c < D / 4; c += 64) {
    const float4 v = x4[c];
    acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
  }
  const float s = dyb_wave_sum(acc);
  if (lane == 0 && want < N) inv_norm[row] = 1.f / fmaxf(sqrtf(s), 1e-8f);
}

template <int NT>
__global__ __launch_bounds__(256, NT == 1 ? 3 : 2) void kmeans_assign_kernel(const float* __restrict__ x, size_t x_stride, const float* __restrict__ x_inv,
                                                            int N, int D, const float* __restrict__ centers,
                                                            const float* __restrict__ c_inv, int K, int* __restrict__ assign,
                                                            float* __restrict__ best, unsigned* __restrict__ changed,
                                                            unsigned* __restrict__ counts, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float Xs[2][KM_ROWS][KM_LD];
  __shared__ __attribute__((aligned(16))) float Cs[2][NT * 32][KM_LD];
  __shared__ float s_invx[KM_ROWS];
  __shared__ float s_best[KM_ROWS];
  __shared__ int s_k[KM_ROWS];
  __shared__ unsigned s_cnt[KM_MAX_K];
  __shared__ unsigned s_changed;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, i32 = lane & 31, half = lane >> 5;
  const long long row0 = (long long)blockIdx.x * KM_ROWS;
  const int sr = t >> 3, sq = t & 7;                                  // staging: rows sr + 32 j, floats 4 sq .. 4 sq + 3 of the step
  const int nsteps = D / KM_STEP;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int i = t; i < K; i += 256) s_cnt[i] = 0u;
  if (t == 0) s_changed = 0u;
  if (t < KM_ROWS) s_invx[t] = row0 + t < N ? x_inv[row0 + t] : 0.f;

  float rbest[16];
  int rk[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { rbest[r] = -INFINITY; rk[r] = 0; }

  float4 gx[2][4], gc[2][NT];                                            // two register sets: the loads run two steps ahead of the MFMAs
  for (int base = 0; base < K; base += NT * 32) {
    auto load = [&](int step, int set) __attribute__((always_inline)) {
      const size_t coff = (size_t)step * KM_STEP + 4 * sq;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long row = row0 + sr + 32 * j;
        gx[set][j] = zero4;
        if (row < N) gx[set][j] = *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(x) + (size_t)row * x_stride + coff * 4);
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int k = base + sr + 32 * j;
        gc[set][j] = zero4;
        if (k < K) gc[set][j] = *reinterpret_cast<const float4*>(centers + (size_t)k * D + coff);
      }
    };
    auto stage = [&](int buf, int set) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(&Xs[buf][sr + 32 * j][4 * sq]) = gx[set][j];
#pragma unroll
      for (int j = 0; j < NT; ++j) *reinterpret_cast<float4*>(&Cs[buf][sr + 32 * j][4 * sq]) = gc[set][j];
    };
    f32x16 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    auto mfma_step = [&](int buf) __attribute__((always_inline)) {
      float4 a[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) a[q] = *reinterpret_cast<const float4*>(&Xs[buf][32 * wave + i32][16 * half + 4 * q]);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        float4 b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = *reinterpret_cast<const float4*>(&Cs[buf][32 * n + i32][16 * half + 4 * q]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].x, b[q].x, acc[n], 0, 0, 0);
          acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].y, b[q].y, acc[n], 0, 0, 0);
          acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].z, b[q].z, acc[n], 0, 0, 0);
          acc[n] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q].w, b[q].w, acc[n], 0, 0, 0);
        }
      }
    };

    load(0, 0);
    if (nsteps > 1) load(1, 1);
    __syncthreads();                                                   // the previous pass has read both LDS stages (and s_invx is set)
    stage(0, 0);
    __syncthreads();
    // two steps per trip, so that LDS stage and register set are constants of each half.  Even half (stage 0): set 1 holds step + 1,
    // set 0 is free for step + 2; the odd half the other way round.  A stage is rewritten only after the barrier behind its last read.
    for (int step = 0; step < nsteps; step += 2) {
      if (step + 2 < nsteps) load(step + 2, 0);
      mfma_step(0);
      if (step + 1 < nsteps) stage(1, 1);
      __syncthreads();
      if (step + 1 >= nsteps) break;
      if (step + 3 < nsteps) load(step + 3, 1);
      mfma_step(1);
      if (step + 2 < nsteps) stage(0, 0);
      __syncthreads();
    }
    // argmax epilogue: accumulator r of a lane is row (r & 3) + 8 (r >> 2) + 4 half of the wave's 32, column i32 of each tile
    float ci[NT];
    int ck[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int k = base + 32 * n + i32;
      ck[n] = k < K ? k : 0x7fffffff;
      ci[n] = k < K ? c_inv[k] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float ix = s_invx[32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half];
      float bc = -INFINITY;
      int bk = 0x7fffffff;
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const float c = ck[n] != 0x7fffffff ? (acc[n][r] * ix) * ci[n] : -INFINITY;
        if (km_better(c, ck[n], bc, bk)) { bc = c; bk = ck[n]; }
      }
#pragma unroll
      for (int m = 16; m >= 1; m >>= 1) {
        const float oc = __shfl_xor(bc, m);
        const int ok = __shfl_xor(bk, m);
        if (km_better(oc, ok, bc, bk)) { bc = oc; bk = ok; }
      }
      if (km_better(bc, bk, rbest[r], rk[r])) { rbest[r] = bc; rk[r] = bk; }
    }
  }
  if (i32 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * half;
      s_best[row] = rbest[r];
      s_k[row] = rk[r];
    }
  }
  __syncthreads();
  if (t < KM_ROWS && row0 + t < N) {
    const int k = s_k[t];                                              // 0 .. K - 1 (a row of NaNs: 0, best -inf)
    const int old = assign[row0 + t];
    assign[row0 + t] = k;
    best[row0 + t] = s_best[t];
    if (old != k) atomicAdd(&s_changed, 1u);
    atomicAdd(&s_cnt[k], 1u);
  }
  __syncthreads();
  for (int i = t; i < K; i += 256)
    if (s_cnt[i]) atomicAdd(&counts[i], s_cnt[i]);
  if (t == 0) {
    if (s_changed) atomicAdd(changed, s_changed);
    double s = 0.0;                                                    // the workgroup's share of the objective, rows in order
    for (int i = 0; i < KM_ROWS && row0 + i < N; ++i) s += (double)s_best[i];
    part[blockIdx.x] = s;
  }
}

// KT clusters per workgroup: 16 KB (KT = 16) or 32 KB of LDS, so that 8 / 5 workgroups share a CU and their row loads - 8 rows in
// flight per thread - cover the memory latency between them.  COMPACT (more than one cluster tile, K > 32): a workgroup meets only
// its own tile's members, a fraction of the chunk, so it first lists them - 2048 rows at a time, every thread scans 8 consecutive
// rows, an exclusive prefix over the 256 counts places them in ascending row order - and then walks the list with every load live.
template <int KT, bool COMPACT>
__global__ __launch_bounds__(256) void kmeans_update_partial_kernel(const float* __restrict__ x, size_t x_stride,
                                                                    const float* __restrict__ x_inv, int N, int D, int K,
                                                                    const int* __restrict__ assign, int R, float* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ float tab[KT][KM_UP_COLS];
  __shared__ unsigned short s_list[COMPACT ? KM_UP_BLOCK : 2];
  __shared__ int s_off[COMPACT ? 257 : 1];
  const int t = threadIdx.x, col = blockIdx.y * KM_UP_COLS + t, k0 = blockIdx.z * KT;
  const bool colok = col < D;
#pragma unroll
  for (int k = 0; k < KT; ++k) tab[k][t] = 0.f;
  const long long r0 = (long long)blockIdx.x * R, r1 = r0 + R < N ? r0 + R : N;
  auto xval = [&](long long row) __attribute__((always_inline)) {
    return reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + (size_t)row * x_stride)[col] * x_inv[row];
  };
  if constexpr (!COMPACT) {
    for (long long i = r0; i < r1; i += KM_UP_UNROLL) {
      int a[KM_UP_UNROLL];
      float v[KM_UP_UNROLL];
#pragma unroll
      for (int j = 0; j < KM_UP_UNROLL; ++j) a[j] = i + j < r1 ? assign[i + j] - k0 : -1;
#pragma unroll
      for (int j = 0; j < KM_UP_UNROLL; ++j) {
        v[j] = 0.f;
        if ((unsigned)a[j] < (unsigned)KT && colok) v[j] = xval(i + j);
      }
#pragma unroll
      for (int j = 0; j < KM_UP_UNROLL; ++j)
        if ((unsigned)a[j] < (unsigned)KT) tab[a[j]][t] += v[j];
    }
  } else {
    for (long long b0 = r0; b0 < r1; b0 += KM_UP_BLOCK) {
      const int nb = r1 - b0 < KM_UP_BLOCK ? (int)(r1 - b0) : KM_UP_BLOCK;
      unsigned mask = 0u;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int row = 8 * t + j;
        if (row < nb && (unsigned)(assign[b0 + row] - k0) < (unsigned)KT) mask |= 1u << j;
      }
      s_off[t + 1] = __builtin_popcount(mask);
      __syncthreads();                                                 // (also: the previous block's list has been walked)
      if (t == 0) {
        s_off[0] = 0;
        for (int i = 1; i <= 256; ++i) s_off[i] += s_off[i - 1];
      }
      __syncthreads();
      int pos = s_off[t];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if ((mask >> j) & 1u) s_list[pos++] = (unsigned short)(8 * t + j);
      __syncthreads();
      const int cnt = s_off[256];
      for (int p = 0; p < cnt; p += KM_UP_UNROLL) {
        int a[KM_UP_UNROLL];
        float v[KM_UP_UNROLL];
#pragma unroll
        for (int j = 0; j < KM_UP_UNROLL; ++j) {
          a[j] = -1;
          v[j] = 0.f;
          if (p + j < cnt) {
            const long long row = b0 + s_list[p + j];
            a[j] = assign[row] - k0;                                   // 0 .. KT - 1: the row is on the list
            if (colok) v[j] = xval(row);
          }
        }
#pragma unroll
        for (int j = 0; j < KM_UP_UNROLL; ++j)
          if (a[j] >= 0) tab[a[j]][t] += v[j];
      }
      __syncthreads();                                                 // the list and the counts are rewritten by the next block
    }
  }
  if (!colok) return;
  for (int k = 0; k < KT && k0 + k < K; ++k) part[((size_t)blockIdx.x * K + k0 + k) * D + col] = tab[k][t];
}

// centre (k, 32 columns) per workgroup: eight groups of 32 threads add the chunk partials g, g + 8, g + 16, ... in that order, group
// sums are added in group order - a fixed tree for given (N, D, K)
__global__ __launch_bounds__(256) void kmeans_update_final_kernel(const float* __restrict__ part, int nchunks, int D, int K,
                                                                  const int* __restrict__ counts, float* __restrict__ centers) {
#pragma clang fp contract(off)
  __shared__ float s_sum[8][32];
  const int k = blockIdx.x, c = threadIdx.x & 31, g = threadIdx.x >> 5, col = blockIdx.y * 32 + c;      // D is a multiple of 32
  const int n = counts[k];
  if (n <= 0) return;                                                  // (the whole workgroup)
  float acc = 0.f;
  for (int ch = g; ch < nchunks; ch += 8) acc += part[((size_t)ch * K + k) * D + col];
  s_sum[g][c] = acc;
  __syncthreads();
  if (g != 0) return;
  float s = s_sum[0][c];
#pragma unroll
  for (int j = 1; j < 8; ++j) s += s_sum[j][c];
  centers[(size_t)k * D + col] = s / (float)n;
}

// rows per chunk of the update, a function of (N, K): at least 16 K rows, so that the partials [chunks][K][D] stay below 1/16 of the
// feature matrix, and at most 512 chunks
static int km_chunk_rows(int N, int K) {
  int r = 16 * K > 64 ? 16 * K : 64;
  if (dyb_cdiv(N, 512) > r) r = dyb_cdiv(N, 512);
  return dyb_cdiv(r, 64) * 64;
}
static bool km_shape_ok(int N, int D, int K) { return N >= 1 && D >= 32 && D % 32 == 0 && K >= 1 && K <= KM_MAX_K; }

extern "C" int dyb_rows_inv_norm(const float* x, size_t x_stride_bytes, int N, int D, float* inv_norm, hipStream_t st) {
  DYB_REQUIRE(x && inv_norm && N >= 1 && D >= 1, DYB_ERR_ARG);
  DYB_REQUIRE(D % 32 == 0, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(((uintptr_t)x & 15) == 0 && (x_stride_bytes & 15) == 0 && x_stride_bytes >= (size_t)D * 4, DYB_ERR_ARG);
  hipLaunchKernelGGL(rows_inv_norm_kernel, dim3(dyb_cdiv(N, 4)), dim3(256), 0, st, x, x_stride_bytes, N, D, inv_norm);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// one fp64 partial of the objective per 128-row workgroup
extern "C" size_t dyb_kmeans_assign_workspace_bytes(int N, int D, int K) {
  if (!km_shape_ok(N, D, K)) return 0;
  return (size_t)dyb_cdiv(N, KM_ROWS) * sizeof(double);
}
// x [N] rows of D floats, row i at x + i * x_stride_bytes (16-byte aligned); x_inv_norm [N], center_inv_norm [K] (dyb_rows_inv_norm);
// centers [K][D].  assign [N] int32 in / out: `changed` counts the rows whose entry differs from the one passed in (fill with -1
// before the first call).  best [N]: the winning cosine.  changed [1] and counts [K] are zeroed and filled by the call.  ws: the
// objective's fp64 partials, sum of best over rows 128 w .. 128 w + 127 at word w: add them in index order on the host.
extern "C" int dyb_kmeans_assign(const float* x, size_t x_stride_bytes, const float* x_inv_norm, int N, int D, const float* centers,
                                 const float* center_inv_norm, int K, int* assign, float* best, int* changed, int* counts, void* ws,
                                 size_t ws_bytes, hipStream_t st) {
  DYB_REQUIRE(x && x_inv_norm && centers && center_inv_norm && assign && best && changed && counts && ws, DYB_ERR_ARG);
  DYB_REQUIRE(N >= 1 && D >= 1 && K >= 1, DYB_ERR_ARG);
  DYB_REQUIRE(D % 32 == 0 && K <= KM_MAX_K, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(((uintptr_t)x & 15) == 0 && (x_stride_bytes & 15) == 0 && x_stride_bytes >= (size_t)D * 4, DYB_ERR_ARG);
  DYB_REQUIRE(((uintptr_t)centers & 15) == 0 && ((uintptr_t)ws & 7) == 0, DYB_ERR_ARG);
  DYB_REQUIRE(ws_bytes >= dyb_kmeans_assign_workspace_bytes(N, D, K), DYB_ERR_WORKSPACE);
  if (hipMemsetAsync(changed, 0, sizeof(int), st) != hipSuccess) return DYB_ERR_LAUNCH;
  if (hipMemsetAsync(counts, 0, (size_t)K * sizeof(int), st) != hipSuccess) return DYB_ERR_LAUNCH;
  const dim3 grid(dyb_cdiv(N, KM_ROWS));
  unsigned* ch = reinterpret_cast<unsigned*>(changed);
  unsigned* cn = reinterpret_cast<unsigned*>(counts);
  double* part = reinterpret_cast<double*>(ws);
  if (K <= 32)
    hipLaunchKernelGGL(kmeans_assign_kernel<1>, grid, dim3(256), 0, st, x, x_stride_bytes, x_inv_norm, N, D, centers, center_inv_norm, K,
                       assign, best, ch, cn, part);
  else if (K <= 64)
    hipLaunchKernelGGL(kmeans_assign_kernel<2>, grid, dim3(256), 0, st, x, x_stride_bytes, x_inv_norm, N, D, centers, center_inv_norm, K,
                       assign, best, ch, cn, part);
  else
    hipLaunchKernelGGL(kmeans_assign_kernel<4>, grid, dim3(256), 0, st, x, x_stride_bytes, x_inv_norm, N, D, centers, center_inv_norm, K,
                       assign, best, ch, cn, part);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// per-chunk partial sums [chunks][K][D] fp32
extern "C" size_t dyb_kmeans_update_workspace_bytes(int N, int D, int K) {
  if (!km_shape_ok(N, D, K)) return 0;
  return (size_t)dyb_cdiv(N, km_chunk_rows(N, K)) * (size_t)K * (size_t)D * sizeof(float);
}
// centers[k] <- (sum over rows i with assign[i] == k of x_i * x_inv_norm[i]) / counts[k]; a row of counts[k] <= 0 is left as it is.
// counts must be the member counts of `assign` (what dyb_kmeans_assign returned, or the host's corrected copy); entries of assign
// outside 0 .. K - 1 belong to no cluster.
extern "C" int dyb_kmeans_update(const float* x, size_t x_stride_bytes, const float* x_inv_norm, int N, int D, const int* assign,
                                 const int* counts, int K, float* centers, void* ws, size_t ws_bytes, hipStream_t st) {
  DYB_REQUIRE(x && x_inv_norm && assign && counts && centers && ws, DYB_ERR_ARG);
  DYB_REQUIRE(N >= 1 && D >= 1 && K >= 1, DYB_ERR_ARG);
  DYB_REQUIRE(D % 32 == 0 && K <= KM_MAX_K, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(((uintptr_t)x & 3) == 0 && (x_stride_bytes & 3) == 0 && x_stride_bytes >= (size_t)D * 4 && ((uintptr_t)ws & 3) == 0, DYB_ERR_ARG);
  DYB_REQUIRE(ws_bytes >= dyb_kmeans_update_workspace_bytes(N, D, K), DYB_ERR_WORKSPACE);
  const int R = km_chunk_rows(N, K), nchunks = dyb_cdiv(N, R), ncolb = dyb_cdiv(D, KM_UP_COLS);
  float* part = reinterpret_cast<float*>(ws);
  if (K <= 16)
    hipLaunchKernelGGL((kmeans_update_partial_kernel<16, false>), dim3(nchunks, ncolb, 1), dim3(256), 0, st, x, x_stride_bytes, x_inv_norm,
                       N, D, K, assign, R, part);
  else if (K <= 32)
    hipLaunchKernelGGL((kmeans_update_partial_kernel<32, false>), dim3(nchunks, ncolb, 1), dim3(256), 0, st, x, x_stride_bytes, x_inv_norm,
                       N, D, K, assign, R, part);
  else
    hipLaunchKernelGGL((kmeans_update_partial_kernel<32, true>), dim3(nchunks, ncolb, dyb_cdiv(K, 32)), dim3(256), 0, st, x,
                       x_stride_bytes, x_inv_norm, N, D, K, assign, R, part);
  DYB_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmeans_update_final_kernel, dim3(K, D / 32), dim3(256), 0, st, (const float*)part, nchunks, D, K, counts, centers);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
