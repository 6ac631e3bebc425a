// Run-time switches of libdynaboa_hip.so, defined once: X(member, name for dyb_set_option / dyb_get_option, environment variable or NULL,
// default, meaning).  Storage, the read of the environment (once, at first use - never on the dispatch path), the name lookup and the DybSw
// enumerators csrc/ reads them through (dyb_switch) are generated from this list in igemm_conv.hip.  Measurements: DESIGN.md section 5.
#pragma once
#define DYB_SWITCH_TABLE(X)                                                                                                                  \
  X(k4, "k4", "DYB_K4", 1, "single-launch 1x1 forward + statistics (latency schedule)")                                                       \
  X(k4_bwd, "k4_bwd", "DYB_K4_BWD", 1, "1x1 data gradient carries the producer's GroupNorm-backward reduce: 1.40 -> 1.31 ms per backward")    \
  X(k4_batch, "k4_batch", "DYB_K4_BATCH", 1, "both single-launch kernels at batch > 1 (up to 64 images)")                                     \
  X(k4_maxc, "k4_maxc", "DYB_K4_MAXC", 1024, "channel limit of the single-launch kernels")                                                    \
  /* replica-aware policy; the throughput schedule: dy materialised once per layer, plain gradient convolutions, no single-launch 1x1 */    \
  X(rep_split, "rep_split", "DYB_REP_SPLIT", 0, "split-K depth chosen for the replica-multiplied grid; throughput schedule from tp_min on")   \
  X(bf16, "bf16", nullptr, 0, "bf16 matrix cores for direct calls of the conv entry points")                                                  \
  X(tp_min, "tp_min", "DYB_TP_MIN", 8, "replicas per launch from which rep_split selects the throughput schedule")                            \
  /* igemm_tp_kernel, 128x128-class tiles */                                                                                                 \
  X(tp_kernel, "tp_kernel", "DYB_TP_KERNEL", 2, "2 software-pipelined loop, 3 two K-steps of loads in flight, 1 phase-separated loop, 0 the 64x64 kernel") \
  X(tp_grid, "tp_grid", "DYB_TP_GRID", 512, "workgroups the throughput kernel's split-K aims for")                                            \
  X(tp_xcd, "tp_xcd", "DYB_TP_XCD", 1, "throughput kernel: XCD-contiguous workgroup order")                                                   \
  /* measured crossover (r05 s17), frames/s latency | throughput at batch 6: 257.7 | 251.0, 8: 280.8 | 294.9, 12: 304.0 | 366.6,            \
     16: 320.9 | 418.6; also the schedule the bf16 form of igemm_tp_kernel needs */                                                          \
  X(tp_batch_min, "tp_batch_min", "DYB_TP_BATCH_MIN", 8, "> 0: the throughput schedule also for single-sequence launches of at least that batch") \
  /* (GroupNorm chunk counts are otherwise sized for one sequence and the launches dispatch-bound) */                                       \
  X(tp_gn_wgs, "tp_gn_wgs", "DYB_TP_GN_WGS", 1024, "workgroups a GroupNorm launch aims for over all replicas under the throughput policy")    \
  X(tp_occ, "tp_occ", "DYB_TP_OCC", 0, "k > 0: at most k workgroups of a throughput launch per CU, through unused dynamic LDS (lab)")         \
  /* throughput GroupNorm backward, one-pass kernel: slabs of several row chunks meet on a counter */                                       \
  X(tp_gn_onepass, "tp_gn_onepass", "DYB_TP_GN_ONEPASS", 2, "2 every layer that qualifies, 1 one-workgroup slabs only, 0 two-launch reduce + apply") \
  X(tp_gn_cap, "tp_gn_cap", "DYB_TP_GN_CAP", 0, "its float4 per workgroup (0: 8 x tp_gn_threads; tests force several chunks on small shapes)") \
  X(tp_gn_threads, "tp_gn_threads", "DYB_TP_GN_THREADS", 1024, "its workgroup size: 256 / 512 / 1024")                                        \
  X(tp_gn_fuse_stats, "tp_gn_fuse_stats", "DYB_TP_GN_FUSE_STATS", 1, "forward GroupNorm statistics leave with the throughput kernel's tiles") \
  X(tp_gn_poll, "tp_gn_poll", "DYB_TP_GN_POLL", 8, "one-pass GroupNorm backward: sleep repetitions between polls of the counter")             \
  X(tp_fwd_nosplit2, "tp_fwd_nosplit2", "DYB_TP_FWD_NOSPLIT2", 1, "a forward split of two runs unsplit when that lets the statistics leave with the tiles") \
  X(pair, "conv_pair", "DYB_CONV_PAIR", 1, "both halves of a tangent pair as one launch of the latency-form kernel")                          \
  X(tp_wt, "tp_wt", "DYB_TP_WT", 1, "cache policy of the throughput kernel's result stores: 0 plain, 1 sc1 write-through, 2 nt, 3 sc0 sc1")    \
  X(tp_stem, "tp_stem", "DYB_TP_STEM", 1, "the stem's forward (Cin = 4) on the throughput kernel's own loader form")                          \
  /* measured (r05 s3): 32 sequences 461 vs 463 frames/s off, 16: 362 vs 376 - the folding workgroups are a tail */                         \
  X(tp_fold, "tp_fold", "DYB_TP_FOLD", 0, "in-kernel split-K fold of the throughput kernel, a bit per mode: 1 forward, 2 data, 4 weight gradient") \
  X(lat_fold, "lat_fold", "DYB_LAT_FOLD", 1, "in-kernel split-K fold of the latency kernel (fp32 form) where a counter region is in scope")   \
  X(stat_folds, "stat_folds", nullptr, 0, "a counter, not a switch: conv launches that folded their split in kernel")                         \
  X(tp_gn_wt, "tp_gn_wt", "DYB_TP_GN_WT", 0, "write-through stores of dy / dm in the one-pass GroupNorm backward")

enum DybSw {
#define DYB_SW_ENUM_(id, name, envname, dflt, doc) DYB_SW_##id,
  DYB_SWITCH_TABLE(DYB_SW_ENUM_)
#undef DYB_SW_ENUM_
  DYB_SW_COUNT
};
