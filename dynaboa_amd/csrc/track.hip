// Person ids for detections that come without them (dynaboa_amd/track.py).  The reference has no tracker - it leaves association to
// external tools: this is the project's own procedure, pinned to the rule at dyb_track_videos in include/dynaboa_hip.h and to its
// fp64 NumPy restatement in tests/track_cases.py.
//
// track_videos_kernel    one workgroup of 256 work-items per video, looping over the video's frames: a frame's association depends
//                        on the tracks the frame before left, so one video is a sequential chain and the parallel axis is the
//                        videos.  All state lives in LDS: the live tracks' keypoints (64 rows of 3 K floats, the row stride made
//                        odd so that a work-item per row walks distinct banks), the frame's detections (the same), the 64 x 64
//                        similarities, and per row a visibility mask (bit k: joint k is visible - `common` is a popcount), area,
//                        last frame id and track id.  Track rows never move: `ord` lists the live rows oldest first, so a track's
//                        place in `ord` orders as its id does and the tie rule needs 6 bits, however large the ids grow.
//                        Per frame: (A) load the detections, work-item 0 retires; (B) a work-item per detection forms mask and
//                        area; (C) a (track, detection) pair per work-item step forms s; (D) greedy rounds - every work-item
//                        takes the maximum of the packed key (s's bits | 63 - place | 63 - index) over its free pairs, a
//                        butterfly and four LDS words make it the workgroup's, work-item 0 marks the pair - until the best is
//                        below s_min; (E) work-item 0 hands the unmatched detections new rows in index order; (F) every matched
//                        or new row takes its detection whole and the ids are written.  Nothing is shared between workgroups
//                        and no order depends on timing: equal bytes from two calls and wherever the video lies in the batch.
#include <math.h>

#include "dyb_common.h"

#define TR_PEOPLE 64               // DYB_TRACK_MAX_PEOPLE of include/dynaboa_hip.h
#define TR_MAX_KP 32               // DYB_TRACK_MAX_KP
#define TR_ROW (3 * TR_MAX_KP + 1)
#define TR_THREADS 256

__device__ __forceinline__ unsigned long long tr_max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// the similarity of two rows: common joints in ascending k, fp32, expf
__device__ __forceinline__ float tr_similarity(const float* t, unsigned tm, float ta, const float* d, unsigned dm, float da, int K,
                                               float kappa, int min_common) {
  const unsigned common = tm & dm;
  const int nc = __builtin_popcount(common);
  if (nc < min_common) return 0.f;
  const float A = fmaxf((ta + da) * 0.5f, 1.f);
  const float den = 2.f * kappa * kappa * A;
  float sum = 0.f;
  for (int k = 0; k < K; ++k) {
    if (!((common >> k) & 1u)) continue;
    const float dx = t[3 * k] - d[3 * k], dy = t[3 * k + 1] - d[3 * k + 1];
    sum += expf(-(dx * dx + dy * dy) / den);
  }
  return sum / (float)nc;
}

__global__ __launch_bounds__(TR_THREADS) void track_videos_kernel(const float* __restrict__ kp, const int* __restrict__ det_offsets,
                                                                  const int* __restrict__ frame_offsets, const int* __restrict__ frame_id,
                                                                  int K, float c_min, float kappa, float s_min, int max_age, int min_common,
                                                                  int* __restrict__ track_out, float* __restrict__ sim_out,
                                                                  int* __restrict__ video_out, int n, int F) {
  __shared__ float t_kp[TR_PEOPLE * TR_ROW];           // track rows
  __shared__ float d_kp[TR_PEOPLE * TR_ROW];           // the frame's detections
  __shared__ float sim[TR_PEOPLE * TR_PEOPLE];         // [place in ord][detection]
  __shared__ unsigned t_mask[TR_PEOPLE], d_mask[TR_PEOPLE];
  __shared__ float t_area[TR_PEOPLE], d_area[TR_PEOPLE], d_sim[TR_PEOPLE];
  __shared__ int t_last[TR_PEOPLE], t_id[TR_PEOPLE], t_used[TR_PEOPLE], t_match[TR_PEOPLE];      // t_match: by place in ord
  __shared__ int ord[TR_PEOPLE], d_match[TR_PEOPLE], d_row[TR_PEOPLE], d_id[TR_PEOPLE];
  __shared__ int live_s;
  __shared__ unsigned long long wave_best[TR_THREADS / 64];

  const int v = blockIdx.x, tid = threadIdx.x;
  const int row = 3 * K | 1;                           // odd: rows a work-item apart start on different banks
  int f0 = frame_offsets[v], f1 = frame_offsets[v + 1];
  f0 = f0 < 0 ? 0 : (f0 > F ? F : f0);
  f1 = f1 < f0 ? f0 : (f1 > F ? F : f1);

  if (tid < TR_PEOPLE) t_used[tid] = 0;
  if (tid == 0) live_s = 0;
  int next_id = 0, started = 0, untrackable = 0, no_slot = 0;            // work-item 0's
  __syncthreads();

  for (int f = f0; f < f1; ++f) {
    int o0 = det_offsets[f], o1 = det_offsets[f + 1];
    o0 = o0 < 0 ? 0 : (o0 > n ? n : o0);
    o1 = o1 < o0 ? o0 : (o1 > n ? n : o1);
    const int nd = o1 - o0, m = nd < TR_PEOPLE ? nd : TR_PEOPLE;
    const int fid = frame_id ? frame_id[f] : f - f0;

    // (A) the frame's first 64 detections -> LDS; the rest get -1 at once; work-item 0 retires
    for (int e = tid; e < m * 3 * K; e += TR_THREADS) {
      const int d = e / (3 * K), c = e - d * 3 * K;
      d_kp[d * row + c] = kp[(size_t)o0 * 3 * K + e];
    }
    for (int d = TR_PEOPLE + tid; d < nd; d += TR_THREADS) {
      track_out[o0 + d] = -1;
      if (sim_out) sim_out[o0 + d] = -1.f;
    }
    if (tid == 0) {
      no_slot += nd - m;
      const int live = live_s;
      int kept = 0;
      for (int r = 0; r < live; ++r) {
        const int slot = ord[r];
        if (fid - t_last[slot] > max_age) t_used[slot] = 0;
        else ord[kept++] = slot;
      }
      live_s = kept;
    }
    __syncthreads();
    const int live = live_s;

    // (B) per detection: visibility, area, whether it can be tracked
    if (tid < m) {
      const float* p = d_kp + tid * row;
      unsigned mask = 0u;
      float x0 = 0.f, x1 = 0.f, y0 = 0.f, y1 = 0.f;
      for (int k = 0; k < K; ++k) {
        if (!(p[3 * k + 2] > c_min)) continue;
        const float x = p[3 * k], y = p[3 * k + 1];
        if (!mask) { x0 = x1 = x; y0 = y1 = y; }
        x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
        mask |= 1u << k;
      }
      const bool ok = __builtin_popcount(mask) >= min_common;
      d_mask[tid] = ok ? mask : 0u;                    // an untrackable detection matches nothing
      d_area[tid] = (x1 - x0) * (y1 - y0);
      d_match[tid] = ok ? -1 : -2;                     // -2: untrackable
      d_sim[tid] = 0.f;
    }
    if (tid < live) t_match[tid] = -1;
    __syncthreads();

    // (C) one (track, detection) pair per work-item step
    const int pairs = live * m;
    for (int p = tid; p < pairs; p += TR_THREADS) {
      const int r = p / m, d = p - r * m, slot = ord[r];
      sim[r * TR_PEOPLE + d] = tr_similarity(t_kp + slot * row, t_mask[slot], t_area[slot], d_kp + d * row, d_mask[d], d_area[d], K, kappa,
                                             min_common);
    }
    __syncthreads();

    // (D) greedy: the largest s among the free pairs, ties to the older track, then to the lower detection index
    const int rounds = live < m ? live : m;
    for (int it = 0; it < rounds; ++it) {
      unsigned long long best = 0ull;
      for (int p = tid; p < pairs; p += TR_THREADS) {
        const int r = p / m, d = p - r * m;
        const float s = sim[r * TR_PEOPLE + d];
        if (s >= s_min && t_match[r] == -1 && d_match[d] == -1)
          best = tr_max64(best, ((unsigned long long)__float_as_uint(s) << 32) | (unsigned long long)(((63 - r) << 6) | (63 - d)));
      }
      best = tr_max64(best, __shfl_xor(best, 32));
      best = tr_max64(best, __shfl_xor(best, 16));
      best = tr_max64(best, __shfl_xor(best, 8));
      best = tr_max64(best, __shfl_xor(best, 4));
      best = tr_max64(best, __shfl_xor(best, 2));
      best = tr_max64(best, __shfl_xor(best, 1));
      if ((tid & 63) == 0) wave_best[tid >> 6] = best;
      __syncthreads();
      best = tr_max64(tr_max64(wave_best[0], wave_best[1]), tr_max64(wave_best[2], wave_best[3]));
      if (best == 0ull) break;                         // the same word for every work-item: the whole workgroup leaves
      if (tid == 0) {
        const int r = 63 - (int)((best >> 6) & 63ull), d = 63 - (int)(best & 63ull);
        t_match[r] = d;
        d_match[d] = r;
        d_sim[d] = __uint_as_float((unsigned)(best >> 32));
      }
      __syncthreads();
    }

    // (E) rows and ids: a matched detection's are its track's; the others start tracks in index order while rows are free
    if (tid == 0) {
      int now = live, free_from = 0;
      for (int d = 0; d < m; ++d) {
        const int r = d_match[d];
        if (r >= 0) {
          d_row[d] = ord[r];
          d_id[d] = t_id[ord[r]];
        } else if (r == -2) {
          d_row[d] = -1; d_id[d] = -1; d_sim[d] = -1.f;
          ++untrackable;
        } else if (now < TR_PEOPLE) {
          while (free_from < TR_PEOPLE - 1 && t_used[free_from]) ++free_from;       // now < 64 rows are in use: a free one exists
          t_used[free_from] = 1;
          t_id[free_from] = next_id;
          ord[now++] = free_from;
          d_row[d] = free_from; d_id[d] = next_id++;
          ++started;
        } else {
          d_row[d] = -1; d_id[d] = -1; d_sim[d] = -1.f;
          ++no_slot;
        }
      }
      live_s = now;
    }
    __syncthreads();

    // (F) a matched or new row takes its detection whole
    for (int e = tid; e < m * 3 * K; e += TR_THREADS) {
      const int d = e / (3 * K), c = e - d * 3 * K, slot = d_row[d];
      if (slot >= 0) t_kp[slot * row + c] = d_kp[d * row + c];
    }
    if (tid < m) {
      const int slot = d_row[tid];
      if (slot >= 0) { t_mask[slot] = d_mask[tid]; t_area[slot] = d_area[tid]; t_last[slot] = fid; }
      track_out[o0 + tid] = d_id[tid];
      if (sim_out) sim_out[o0 + tid] = d_sim[tid];
    }
    __syncthreads();
  }

  if (tid == 0) {
    video_out[4 * v + 0] = started;
    video_out[4 * v + 1] = untrackable;
    video_out[4 * v + 2] = no_slot;
    video_out[4 * v + 3] = 0;
  }
}

extern "C" int dyb_track_videos(const float* kp, const int* det_offsets, const int* frame_offsets, const int* frame_id, int K, float c_min,
                                float kappa, float s_min, int max_age, int min_common, int* track_out, float* sim_out, int* video_out,
                                int n, int F, int V, hipStream_t st) {
  DYB_REQUIRE(n >= 0 && F >= 0 && V >= 1, DYB_ERR_ARG);
  DYB_REQUIRE(K >= 1 && K <= TR_MAX_KP && max_age >= 0 && min_common >= 1, DYB_ERR_ARG);
  DYB_REQUIRE(std::isfinite(c_min) && std::isfinite(kappa) && std::isfinite(s_min), DYB_ERR_ARG);
  DYB_REQUIRE(kappa > 0.f && s_min > 0.f && s_min <= 1.f, DYB_ERR_ARG);
  DYB_REQUIRE(det_offsets && frame_offsets && video_out, DYB_ERR_ARG);
  DYB_REQUIRE(n == 0 || (kp && track_out), DYB_ERR_ARG);
  hipLaunchKernelGGL(track_videos_kernel, dim3((unsigned)V), dim3(TR_THREADS), 0, st, kp, det_offsets, frame_offsets, frame_id, K, c_min, kappa,
                     s_min, max_age, min_common, track_out, sim_out, video_out, n, F);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
