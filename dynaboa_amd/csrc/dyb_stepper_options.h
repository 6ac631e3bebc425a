// Options of the native frame stepper (adapt_step.hip), defined once: X(Stepper member, key for dyb_stepper_set_i / _f / _p and
// dyb_stepper_get_i / _f, environment variable or NULL, type I int | F double | P pointer, locked once the workspace is bound, meaning).
// The name lookup of the setters and getters and the environment reads in dyb_stepper_create (int rows; a later set_i wins) are
// generated from this list; defaults and the longer notes sit with the members in struct Stepper.  Keys with code of their own:
// "adam_step", "adam_step_<replica>", "bank_seed", "bank_draw_<replica>", "drop_seed", "drop_offset", "replicas" (locked), "logs_bytes", "result_floats" (get_i: B * 20900), the "smpl_*" / "smpli_*" table
// families and the range check of "drop_p" (0 <= p < 1).  Measurements: DESIGN.md section 5.
#pragma once
#define DYB_STEPPER_OPTIONS_I(X)                                                                                                              \
  X(n_iter, "n_iter", nullptr, I, 0, "iterations of the HMR regressor (1 .. 3)")                                                              \
  X(inner_step, "inner_step", nullptr, I, 0, "lower levels per frame (0 .. 16)")                                                              \
  X(eval_lower, "eval_lower", nullptr, I, 0, "a metric record after every inner step")                                                        \
  X(use_side, "use_side", nullptr, I, 0, "frame-loss set: final inference and ground-truth meshes on the side stream (groups: with group_side)") \
  X(metrics, "metrics", nullptr, I, 0, "metric records at all")                                                                               \
  X(upd_overlap, "upd_overlap", "DYB_UPD_OVERLAP", I, 0, "replica groups: weight updates by arena ranges beside the next forward")            \
  X(upd_late, "upd_late", "DYB_UPD_LATE", I, 0, "the last range (layer4 + regressor) is issued when the consuming forward reaches layer3")    \
  X(wgrad_defer, "wgrad_defer", "DYB_WGRAD_DEFER", I, 0, "layer4 / regressor weight gradients behind the backward's join, beside the next forward") \
  X(group_side, "group_side", "DYB_GROUP_SIDE", I, 0, "replica groups, frame-loss set: the final inference on the side stream, beside the next frame's first level") \
  X(fuse_fast, "fuse_fast", "DYB_FUSE_FAST", I, 1, "frame-loss set: lower levels' weight gradients write the fast weights themselves (second fast buffer)") \
  X(fuse_adam, "fuse_adam", "DYB_FUSE_ADAM", I, 0, "frame-loss set, replica groups: the outer level's weight gradients apply Adam in place")  \
  X(fuse_ema, "fuse_ema", "DYB_FUSE_EMA", I, 0, "the teacher's EMA inside the Adam pass")                                                     \
  X(par_passes, "par_passes", "DYB_PAR_PASSES", I, 0, "full set: history and exemplar passes on two streams of the stepper's own")            \
  X(par_max_replicas, "par_max_replicas", "DYB_PAR_MAX_REPLICAS", I, 0, "largest launch set that still runs the parallel passes")             \
  X(share_dyn_fwd, "share_dyn_fwd", "DYB_SHARE_DYN_FWD", I, 0, "dynamic loop: a step's upper level reuses the previous final inference as its forward") \
  X(full, "full", nullptr, I, 1, "the reference's full term set (teacher / motion / labelled exemplars / dynamic loop): sizes the workspace")  \
  X(temporal_lower, "temporal_lower", nullptr, I, 0, "teacher / motion terms on the lower levels")                                            \
  X(temporal_upper, "temporal_upper", nullptr, I, 0, "teacher / motion terms on the upper level")                                             \
  X(use_teacher, "use_teacher", nullptr, I, 0, "mean-teacher term and the teacher's EMA")                                                     \
  X(teacher_train, "teacher_train", nullptr, I, 0, "teacher forwards with live dropout (keys: drop_seed, drop_offset)")                       \
  X(use_motion, "use_motion", nullptr, I, 0, "motion term against the frame `interval` steps back")                                           \
  X(interval, "interval", nullptr, I, 0, "distance of the history frame (bookkeeping of the caller)")                                         \
  X(mix_lower, "mix_lower", nullptr, I, 0, "labelled-exemplar term on the lower levels")                                                      \
  X(mix_upper, "mix_upper", nullptr, I, 0, "labelled-exemplar term on the upper level")                                                       \
  X(dynamic, "dynamic", nullptr, I, 0, "dynamic loop: repeat the upper level while feature 12 still moves")                                   \
  X(optim_steps, "optim_steps", nullptr, I, 0, "its iteration limit")                                                                         \
  X(kp_set, "kp_set", nullptr, I, 0, "keypoint window of the 2D term and the motion term: 0 gt24 (joints 25..48) | 1 op25 (joints 0..24)")   \
  X(record_capacity, "record_capacity", nullptr, I, 0, "metric-record slots behind `records`")                                                \
  X(loss_capacity, "loss_capacity", nullptr, I, 0, "frames behind `loss_log` / `gate_log`")                                                   \
  X(result_capacity, "result_capacity", nullptr, I, 0, "rows behind `results` (a frame's final inferences go to row loss_slot mod this)")      \
  X(bank_items, "bank_items", nullptr, I, 0, "exemplar bank: items in the five tables")                                                       \
  X(bank_clusters, "bank_clusters", nullptr, I, 0, "exemplar bank: cluster centres")                                                          \
  X(bank_members, "bank_members", nullptr, I, 0, "exemplar bank: entries of bank_member_idx")                                                 \
  X(bank_pick_capacity, "bank_pick_capacity", nullptr, I, 0, "exemplar bank: rows of each replica's pick log (row = draw index mod this)")    \
  X(bank_on_device, "bank_on_device", "DYB_BANK_ON_DEVICE", I, 0, "exemplar bank: 1 select / gather kernels inside the level | 0 ignore the bank (callback route; A/B)")
#define DYB_STEPPER_OPTIONS_F(X)                                                                                                              \
  X(lr, "lr", nullptr, F, 0, "Adam learning rate")                                                                                            \
  X(beta1, "beta1", nullptr, F, 0, "Adam beta1")                                                                                              \
  X(beta2, "beta2", nullptr, F, 0, "Adam beta2")                                                                                              \
  X(eps, "eps", nullptr, F, 0, "Adam epsilon")                                                                                                \
  X(fastlr, "fastlr", nullptr, F, 0, "fast-weight learning rate")                                                                             \
  X(w2d, "s2dloss_weight", nullptr, F, 0, "frame head: 2D keypoint term")                                                                     \
  X(wshape, "shape_prior_weight", nullptr, F, 0, "frame head: shape prior")                                                                   \
  X(wpose, "pose_prior_weight", nullptr, F, 0, "frame head: pose prior")                                                                      \
  X(teacher_w, "teacherloss_weight", nullptr, F, 0, "weight of the teacher term")                                                             \
  X(motion_w, "motionloss_weight", nullptr, F, 0, "weight of the motion term")                                                                \
  X(label_w, "labelloss_weight", nullptr, F, 0, "weight of the labelled term")                                                                \
  X(alpha, "alpha", nullptr, F, 0, "teacher EMA: t = alpha * t + (1 - alpha) * theta")                                                        \
  X(cos_thr, "cos_sim_threshold", nullptr, F, 0, "dynamic loop goes on while 1 - cos(feature 12) exceeds it")                                 \
  X(drop_p, "drop_p", nullptr, F, 0, "teacher dropout probability")
#define DYB_STEPPER_OPTIONS_P(X)                                                                                                              \
  X(theta, "theta", nullptr, P, 0, "[replicas][param floats] weights")                                                                        \
  X(adam_m, "adam_m", nullptr, P, 0, "[replicas][param floats] Adam exp_avg")                                                                 \
  X(adam_v, "adam_v", nullptr, P, 0, "[replicas][param floats] Adam exp_avg_sq")                                                              \
  X(init_state, "init_state", nullptr, P, 0, "[B][160] initial regressor state")                                                              \
  X(gmm_means, "gmm_means", nullptr, P, 0, "pose prior: means")                                                                               \
  X(gmm_prec, "gmm_precisions", nullptr, P, 0, "pose prior: precisions")                                                                      \
  X(gmm_logw, "gmm_log_weights", nullptr, P, 0, "pose prior: log weights")                                                                    \
  X(j_h36m, "j_regressor_h36m", nullptr, P, 0, "[17][6890] joint regressor of the metrics")                                                   \
  X(j14, "j14", nullptr, P, 0, "[14] int: H36M -> J14 joint map")                                                                             \
  X(logs_base, "logs_base", nullptr, P, 0, "one per-replica block holding records | loss_log | gate_log | feat5_out | results (with logs_bytes)")       \
  X(records, "records", nullptr, P, 0, "[replicas][record_capacity][record_floats]")                                                          \
  X(loss_log, "loss_log", nullptr, P, 0, "[replicas][loss_capacity][loss_floats]")                                                            \
  X(teacher, "teacher", nullptr, P, 0, "[replicas][param floats] teacher weights")                                                            \
  X(gate_host, "gate_host", nullptr, P, 0, "pinned host memory, 16 floats per replica: the gate's cosines + sequence number")                 \
  X(gate_log, "gate_log", nullptr, P, 0, "[replicas][loss_capacity][1 + optim_steps][16] cosines of every gate evaluation")                   \
  X(feat5_out, "feat5_out", nullptr, P, 0, "[replicas][B][2048] pooled feature handed to the retrieval callback")                             \
  X(results, "results", nullptr, P, 0, "[replicas][result_capacity][result_floats] result ring: each replica's last final inference of a frame") \
  X(retrieve, "retrieve_fn", nullptr, P, 0, "int (*)(user, level, out[5]): exemplars of one sequence")                                        \
  X(retrieve_rep, "retrieve_rep_fn", nullptr, P, 0, "int (*)(user, level, physical replica, out[5]): exemplars of a replica")                 \
  X(retrieve_user, "retrieve_user", nullptr, P, 0, "first argument of the callbacks")                                                         \
  X(bank_img, "bank_img", nullptr, P, 0, "exemplar bank: [items][3][224][224] crops")                                                         \
  X(bank_kp, "bank_keypoints", nullptr, P, 0, "exemplar bank: [items][49][3]")                                                                \
  X(bank_pose, "bank_pose", nullptr, P, 0, "exemplar bank: [items][72]")                                                                      \
  X(bank_betas, "bank_betas", nullptr, P, 0, "exemplar bank: [items][10]")                                                                    \
  X(bank_pose3d, "bank_pose_3d", nullptr, P, 0, "exemplar bank: [items][24][4]")                                                              \
  X(bank_centers, "bank_centers", nullptr, P, 0, "exemplar bank: [clusters][2048] centres")                                                   \
  X(bank_inv_norm, "bank_center_inv_norm", nullptr, P, 0, "exemplar bank: [clusters] 1 / |centre|")                                           \
  X(bank_member_ptr, "bank_member_ptr", nullptr, P, 0, "exemplar bank: [clusters + 1] int, CSR offsets of the clusters' members")             \
  X(bank_member_idx, "bank_member_idx", nullptr, P, 0, "exemplar bank: [members] int, item indices")                                          \
  X(bank_picks, "bank_picks", nullptr, P, 0, "[replicas][bank_pick_capacity][2] int: (cluster, item) of every draw")
