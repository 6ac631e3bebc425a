// Native HMR engine: a static execution plan for the ResNet-50(GN) backbone + 3-iteration SMPL
// regressor of reference model/hmr.py:63-181, forward and backward, over
//   * ONE flat fp32 parameter arena (conv weights re-laid [R][S][Cin][Cout], fc1 rows padded to
//     2208, the three decoder heads fused into one [160][1024] matrix),
//   * ONE activation arena per forward call: every raw conv output y (what backward needs) plus the
//     block outputs; the GroupNorm+ReLU outputs INSIDE a bottleneck (bn1, bn2, downsample.1) have a
//     single consumer and are never written - that consumer normalises y on the fly in its loader,
//   * a workspace (split-K slabs, norm partials, three gradient buffers, per-layer masked gradients).
// One C call = one whole forward (112 launches: conv -> statistics per layer - one launch for the small 1x1
// layers -, one apply per block output) or backward (~210: GroupNorm-backward reduce -> data gradient per layer on the critical
// chain, weight gradients on an auxiliary stream), no host syncs, no allocation, capturable in a
// hipGraph.  PyTorch only owns the memory and the stream.
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "dyb_common.h"
#include "dyb_philox.h"

// ---- low-level entry points defined in the sibling files -----------------------------------
extern "C" {
size_t dyb_conv2d_workspace_bytes(int, int, int, int, int, int, int, int, int);
size_t dyb_groupnorm_workspace_bytes(int, int, int);
int dyb_conv2d_nhwc_fwd_gnstats(const float*, const float*, int, const float*, const float*, int, float*, const float*, float*,
                                float*, int*, int, int, int, int, int, int, int, int, int, void*, size_t, hipStream_t);
int dyb_groupnorm_apply_n(const float*, const float*, int, const float*, const float*, const float*, const float*, int,
                          const float*, const float*, float*, float*, float*, int, int, int, int, hipStream_t);
int dyb_conv2d_nhwc_wgrad_gn_n(const float*, const float*, const float*, const float*, const float*, const float*, const float*,
                               const float*, const float*, int, int, const float*, float*, float*, float*, int, int, int, int,
                               int, int, int, int, int, void*, size_t, hipStream_t);
size_t dyb_groupnorm_bwd_partial_floats(int, int, int);
int dyb_conv2d_nhwc_dgrad_gn(const float*, const float*, const float*, const float*, const float*, const float*, float*,
                             const float*, int, int, int, int, int, int, int, int, int, void*, size_t, hipStream_t);
int dyb_conv2d_nhwc_wgrad_gn(const float*, const float*, const float*, const float*, const float*, const float*, float*,
                             float*, float*, int, int, int, int, int, int, int, int, int, void*, size_t, hipStream_t);
int dyb_nchw3_to_nhwc4(const float*, float*, int, int, int, hipStream_t);
int dyb_maxpool3x3s2_fwd(const float*, float*, uint32_t*, int, int, int, int, hipStream_t);
int dyb_maxpool3x3s2_bwd(const float*, const uint32_t*, float*, int, int, int, int, hipStream_t);
int dyb_avgpool_fwd(const float*, float* const*, int, int, int, int, int, hipStream_t);
int dyb_avgpool_bwd(const float*, int, float*, int, int, int, hipStream_t);
int dyb_linear_fwd(const float*, int, const float*, int, const float*, const float*, int, float*, int, int, int, int,
                   hipStream_t);
size_t dyb_linear_bwd_workspace_bytes(int, int, int);
int dyb_linear_bwd_dx(const float*, int, const float*, int, int, int, int, float*, int, int, int, float*, int,
                      const float*, int, void*, size_t, hipStream_t);
int dyb_linear_bwd_dw(const float* const*, const int*, const float* const*, const int*, int, int, int, int, float*, int,
                      float*, hipStream_t);
int dyb_rot6d_fwd(const float*, int, float*, int, hipStream_t);
int dyb_rot6d_bwd(const float*, int, const float*, float*, int, int, hipStream_t);
int dyb_scale_add(const float*, const float*, const float*, float*, size_t, hipStream_t);
}

#define FC1_IN_PAD 2208
#define FEAT 2048
#define STATE_LD 160     // pose 144 | shape 10 | cam 3 | pad 3
#define HID 1024
#define MAX_ITER 3
#define SYNC_WORDS 8

enum TensorKind { K_CONV_W = 0, K_NORM_W = 1, K_NORM_B = 2, K_FC_W = 3, K_FC_B = 4, K_DEC_W = 5, K_DEC_B = 6 };

struct TensorInfo {
  std::string name;
  int kind;
  size_t offset;     // floats into the parameter arena
  int dims[4];       // conv: Cout,Cin(reference),R,S ; fc: out,in(reference),ld,0 ; norm: C
  int cin_pad;
};

struct ConvL {
  int H, W, C, K, R, S, stride, pad, Ho, Wo;
  size_t w, gam, bet;          // parameter offsets
  size_t y, out, stats;        // activation offsets (conv output, normalised output, [B][4][2])
  bool has_out;                // false: the normalised output is never materialised (out is invalid)
  size_t dy;                   // offset (floats) of this layer's masked GroupNorm-output gradient in the workspace dm arena
  size_t gnb;                  // offset (floats) of this layer's GroupNorm-backward partial sums in the workspace
};
struct BlockL {
  int c1, c2, c3, cd;          // indices into convs (cd = -1: identity shortcut)
};

struct GKey {
  uintptr_t a[10];
  bool operator==(const GKey& o) const { return memcmp(a, o.a, sizeof(a)) == 0; }
};
struct GKeyHash {
  size_t operator()(const GKey& k) const {
    size_t h = 1469598103934665603ull;
    for (uintptr_t v : k.a) { h ^= (size_t)v; h *= 1099511628211ull; }
    return h;
  }
};
struct GEntry {
  hipGraphExec_t exec = nullptr;
  int seen = 0;
  bool bad = false;
};
#define DYB_MAX_GRAPHS 96

struct HmrPlan {
  int B, H, W;
  std::vector<ConvL> convs;
  std::vector<BlockL> blocks;
  int layer_last_block[4];
  std::vector<TensorInfo> tensors;
  size_t n_params;
  size_t fc1_w, fc1_b, fc2_w, fc2_b, dec_w, dec_b;
  // activation arena
  size_t a_x4, a_pool, a_poolidx, a_xc[MAX_ITER], a_h1[MAX_ITER], a_h2[MAX_ITER], a_state, a_rot;
  size_t a_h1d[MAX_ITER], a_h2d[MAX_ITER];      // train mode only: the hidden vectors after nn.Dropout (model/hmr.py:165,169)
  size_t act_floats;
  int poolH, poolW;            // max-pool output
  int featHW;                  // spatial size of the last feature map (7*7)
  // workspace carve (bytes)
  size_t ws_conv, ws_conv_aux, ws_gn, ws_gnb, ws_lin, ws_grad_each, ws_dy, ws_dy2, ws_reg, ws_sync, ws_total;
  // hipGraph cache: a whole forward / backward call is captured once per distinct set of pointer
  // arguments (the caching allocator reproduces addresses in a steady-state frame loop) and replayed
  // with ONE hipGraphLaunch instead of ~180 / ~330 launches: the eager loop is host-issue-bound.
  int graph_mode;
  int bf16;                    // convolutions of this plan run on the bf16 matrix cores (operands rounded when staged; fp32 everywhere else)
  int fold_in_reduce;          // leave data-gradient split-K slabs for the next GroupNorm-backward reduce to fold
  long g_hits, g_eager, g_captures, g_fail_begin, g_fail_body, g_fail_end, g_fail_inst, g_fail_launch;
  // cross-stream ordering for the weight-gradient convolutions (created on first use): the plan's own set serves the
  // dyb_hmr_backward entry point; a caller that runs several backward chains of one plan concurrently (replica
  // streams of the native frame stepper) brings one set per chain (dyb_hmr_events_create)
  DybEvents ev;
  bool events_ready;
  std::unordered_map<GKey, GEntry, GKeyHash> gfwd, gbwd;
  // one plan serves every stream / host thread of the process (metric worker, replica threads): the lazily created
  // events and the graph cache are the only mutable state and sit behind this lock (the eager path never takes it)
  std::mutex mu;
};

static size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }

static int add_conv(HmrPlan& P, const std::string& cname, const std::string& nname, int H, int W, int Cin_ref, int Cout,
                    int k, int stride, int pad, size_t& poff, size_t& aoff, bool keep_out) {
  ConvL c{};
  int cin_pad = Cin_ref < 4 ? 4 : Cin_ref;
  c.H = H; c.W = W; c.C = cin_pad; c.K = Cout; c.R = k; c.S = k; c.stride = stride; c.pad = pad;
  c.Ho = (H + 2 * pad - k) / stride + 1;
  c.Wo = (W + 2 * pad - k) / stride + 1;
  c.w = poff;
  P.tensors.push_back({cname + ".weight", K_CONV_W, poff, {Cout, Cin_ref, k, k}, cin_pad});
  poff = align64(poff + (size_t)k * k * cin_pad * Cout);
  c.gam = poff;
  P.tensors.push_back({nname + ".weight", K_NORM_W, poff, {Cout, 0, 0, 0}, 0});
  poff = align64(poff + Cout);
  c.bet = poff;
  P.tensors.push_back({nname + ".bias", K_NORM_B, poff, {Cout, 0, 0, 0}, 0});
  poff = align64(poff + Cout);
  size_t n = (size_t)P.B * c.Ho * c.Wo * Cout;
  c.y = aoff; aoff = align64(aoff + n);
  c.has_out = keep_out;
  c.out = aoff;
  if (keep_out) aoff = align64(aoff + n);
  c.stats = aoff; aoff = align64(aoff + (size_t)P.B * DYB_GN_GROUPS * 2);
  P.convs.push_back(c);
  return (int)P.convs.size() - 1;
}

static HmrPlan* build_plan(int B, int H, int W) {
  HmrPlan* pp = new HmrPlan();
  HmrPlan& P = *pp;
  P.B = B; P.H = H; P.W = W;
  size_t poff = 0, aoff = 0;
  P.a_x4 = aoff; aoff = align64(aoff + (size_t)B * H * W * 4);
  int stem = add_conv(P, "conv1", "bn1", H, W, 3, 64, 7, 2, 3, poff, aoff, true);
  int h = P.convs[stem].Ho, w = P.convs[stem].Wo;
  P.poolH = (h + 2 - 3) / 2 + 1;
  P.poolW = (w + 2 - 3) / 2 + 1;
  P.a_pool = aoff; aoff = align64(aoff + (size_t)B * P.poolH * P.poolW * 64);
  P.a_poolidx = aoff; aoff = align64(aoff + (size_t)B * P.poolH * P.poolW * 16);   // uint32 per float4
  h = P.poolH; w = P.poolW;
  const int nblocks[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512};
  int inplanes = 64;
  for (int li = 0; li < 4; ++li) {
    for (int bi = 0; bi < nblocks[li]; ++bi) {
      std::string pre = "layer" + std::to_string(li + 1) + "." + std::to_string(bi) + ".";
      int stride = (bi == 0 && li > 0) ? 2 : 1;
      BlockL b{};
      b.c1 = add_conv(P, pre + "conv1", pre + "bn1", h, w, inplanes, planes[li], 1, 1, 0, poff, aoff, false);
      b.c2 = add_conv(P, pre + "conv2", pre + "bn2", h, w, planes[li], planes[li], 3, stride, 1, poff, aoff, false);
      int h2 = P.convs[b.c2].Ho, w2 = P.convs[b.c2].Wo;
      b.c3 = add_conv(P, pre + "conv3", pre + "bn3", h2, w2, planes[li], planes[li] * 4, 1, 1, 0, poff, aoff, true);
      b.cd = -1;
      if (bi == 0)
        b.cd = add_conv(P, pre + "downsample.0", pre + "downsample.1", h, w, inplanes, planes[li] * 4, 1, stride, 0, poff,
                        aoff, false);
      P.blocks.push_back(b);
      inplanes = planes[li] * 4;
      h = h2; w = w2;
    }
    P.layer_last_block[li] = (int)P.blocks.size() - 1;
  }
  P.featHW = h * w;
  P.fc1_w = poff; P.tensors.push_back({"fc1.weight", K_FC_W, poff, {HID, FEAT + 157, FC1_IN_PAD, 0}, 0});
  poff = align64(poff + (size_t)HID * FC1_IN_PAD);
  P.fc1_b = poff; P.tensors.push_back({"fc1.bias", K_FC_B, poff, {HID, 0, 0, 0}, 0});
  poff = align64(poff + HID);
  P.fc2_w = poff; P.tensors.push_back({"fc2.weight", K_FC_W, poff, {HID, HID, HID, 0}, 0});
  poff = align64(poff + (size_t)HID * HID);
  P.fc2_b = poff; P.tensors.push_back({"fc2.bias", K_FC_B, poff, {HID, 0, 0, 0}, 0});
  poff = align64(poff + HID);
  P.dec_w = poff; P.tensors.push_back({"dec.weight", K_DEC_W, poff, {STATE_LD, HID, HID, 0}, 0});
  poff = align64(poff + (size_t)STATE_LD * HID);
  P.dec_b = poff; P.tensors.push_back({"dec.bias", K_DEC_B, poff, {STATE_LD, 0, 0, 0}, 0});
  poff = align64(poff + STATE_LD);
  P.n_params = poff;
  for (int t = 0; t < MAX_ITER; ++t) {
    P.a_xc[t] = aoff; aoff = align64(aoff + (size_t)B * FC1_IN_PAD);
    P.a_h1[t] = aoff; aoff = align64(aoff + (size_t)B * HID);
    P.a_h2[t] = aoff; aoff = align64(aoff + (size_t)B * HID);
    P.a_h1d[t] = aoff; aoff = align64(aoff + (size_t)B * HID);
    P.a_h2d[t] = aoff; aoff = align64(aoff + (size_t)B * HID);
  }
  P.a_state = aoff; aoff = align64(aoff + (size_t)B * STATE_LD);
  P.a_rot = aoff; aoff = align64(aoff + (size_t)B * 24 * 9);
  P.act_floats = aoff;

  size_t wc = 0, wg = 0, maxact = 0, dyoff = 0, gnboff = 0;
  P.events_ready = false;
  P.graph_mode = 0;
  P.bf16 = 0;
  {
    const char* e = getenv("DYB_FOLD_IN_REDUCE");
    P.fold_in_reduce = e ? atoi(e) : 1;     // measured 1.55 vs 1.75 ms per backward
  }
  P.g_hits = P.g_eager = P.g_captures = 0;
  P.g_fail_begin = P.g_fail_body = P.g_fail_end = P.g_fail_inst = P.g_fail_launch = 0;
  for (auto& c : P.convs) {
    c.dy = dyoff;
    dyoff = align64(dyoff + (size_t)B * c.Ho * c.Wo * c.K);
    c.gnb = gnboff;
    gnboff = align64(gnboff + dyb_groupnorm_bwd_partial_floats(B, c.Ho * c.Wo, c.K));
    size_t s = dyb_conv2d_workspace_bytes(B, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad);
    if (s > wc) wc = s;
    size_t g = dyb_groupnorm_workspace_bytes(B, c.Ho * c.Wo, c.K);
    if (g > wg) wg = g;
    size_t n = (size_t)B * c.Ho * c.Wo * c.K;
    if (n > maxact) maxact = n;
    size_t nin = (size_t)B * c.H * c.W * c.C;
    if (nin > maxact) maxact = nin;
  }
  size_t wl = dyb_linear_bwd_workspace_bytes(B, FC1_IN_PAD, HID);
  size_t wl2 = dyb_linear_bwd_workspace_bytes(B, HID, HID);
  if (wl2 > wl) wl = wl2;
  P.ws_conv = align64(wc / 4) * 4;
  P.ws_conv_aux = P.ws_conv;
  P.ws_dy = dyoff * 4;
  P.ws_dy2 = dyoff * 4;         // per-layer dy slots of the throughput schedule (materialised GroupNorm-backward outputs)
  P.ws_gn = align64(wg / 4) * 4;
  P.ws_gnb = gnboff * 4;
  P.ws_lin = align64(wl / 4) * 4;
  P.ws_grad_each = align64(maxact) * 4;
  // regressor gradient scratch: d_st[4][B][160], d_h2[3][B][1024], d_h1[3][B][1024], d_xc[B][2208], two [B][1024] for sum_t d_h1[t]
  P.ws_reg = align64((size_t)B * (4 * STATE_LD + 8 * HID + FC1_IN_PAD)) * 4;
  // arrival counters of the one-pass GroupNorm backward: SYNC_WORDS per conv layer (4 groups + the error word), zeroed per backward
  // + two counter regions of the convolutions' in-kernel split-K fold (chain stream | auxiliary stream), zeroed per pass
  P.ws_sync = (align64(P.convs.size() * SYNC_WORDS) + 2 * (size_t)DYB_CONV_SYNC_WORDS) * 4;
  P.ws_total = P.ws_conv + P.ws_conv_aux + 3 * P.ws_gn + P.ws_gnb + P.ws_lin + 3 * P.ws_grad_each + P.ws_dy + P.ws_reg + P.ws_dy2 + P.ws_sync;
  return pp;
}

extern "C" int dyb_hmr_plan_create(int B, int H, int W, void** plan) {
  DYB_REQUIRE(plan && B > 0 && B <= 64 && H > 0 && W > 0, DYB_ERR_ARG);
  HmrPlan* p = build_plan(B, H, W);
  *plan = p;
  return DYB_OK;
}
extern "C" void dyb_hmr_plan_destroy(void* plan) {
  HmrPlan* P = reinterpret_cast<HmrPlan*>(plan);
  if (!P) return;
  if (P->events_ready) {
    for (hipEvent_t e : P->ev.dy) (void)hipEventDestroy(e);
    (void)hipEventDestroy(P->ev.join);
  }
  for (auto& kv : P->gfwd) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  for (auto& kv : P->gbwd) if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
  delete P;
}
#define RUN_RC(x)                \
  do {                           \
    int rc__ = (x);              \
    if (rc__ != DYB_OK) return rc__; \
  } while (0)
static int fill_events(const HmrPlan& P, DybEvents& e) {
  e.dy.resize(P.convs.size());
  for (size_t i = 0; i < P.convs.size(); ++i)
    if (hipEventCreateWithFlags(&e.dy[i], hipEventDisableTiming) != hipSuccess) return DYB_ERR_LAUNCH;
  if (hipEventCreateWithFlags(&e.join, hipEventDisableTiming) != hipSuccess) return DYB_ERR_LAUNCH;
  return DYB_OK;
}
static int ensure_events(HmrPlan& P) {
  std::lock_guard<std::mutex> lock(P.mu);
  if (P.events_ready) return DYB_OK;
  RUN_RC(fill_events(P, P.ev));
  P.events_ready = true;
  return DYB_OK;
}
DybEvents* dyb_hmr_events_create(const void* plan) {
  const HmrPlan* P = reinterpret_cast<const HmrPlan*>(plan);
  if (!P) return nullptr;
  DybEvents* e = new DybEvents();
  if (fill_events(*P, *e) != DYB_OK) { delete e; return nullptr; }
  return e;
}
void dyb_hmr_events_destroy(DybEvents* e) {
  if (!e) return;
  for (hipEvent_t x : e->dy) (void)hipEventDestroy(x);
  (void)hipEventDestroy(e->join);
  if (e->l4) (void)hipEventDestroy(e->l4);
  if (e->reg) (void)hipEventDestroy(e->reg);
  delete e;
}
extern "C" size_t dyb_hmr_param_floats(const void* plan) { return reinterpret_cast<const HmrPlan*>(plan)->n_params; }
extern "C" size_t dyb_hmr_act_floats(const void* plan) { return reinterpret_cast<const HmrPlan*>(plan)->act_floats; }
extern "C" size_t dyb_hmr_workspace_bytes(const void* plan) { return reinterpret_cast<const HmrPlan*>(plan)->ws_total; }
extern "C" int dyb_hmr_num_tensors(const void* plan) { return (int)reinterpret_cast<const HmrPlan*>(plan)->tensors.size(); }
extern "C" int dyb_hmr_tensor_info(const void* plan, int i, char* name, int name_cap, int* kind, long long* offset,
                                   int* dims4, int* cin_pad) {
  const HmrPlan* P = reinterpret_cast<const HmrPlan*>(plan);
  DYB_REQUIRE(P && i >= 0 && i < (int)P->tensors.size() && name && kind && offset && dims4 && cin_pad, DYB_ERR_ARG);
  const TensorInfo& t = P->tensors[i];
  strncpy(name, t.name.c_str(), name_cap - 1);
  name[name_cap - 1] = 0;
  *kind = t.kind; *offset = (long long)t.offset; *cin_pad = t.cin_pad;
  for (int k = 0; k < 4; ++k) dims4[k] = t.dims[k];
  return DYB_OK;
}
// Activation-arena locations of the 15 "features" of HMR.forward(need_feature=True)
// (reference model/hmr.py:139-168).  which: 0 = conv1 output, 1..4 = layer1..4 outputs (NHWC),
// 5 = pooled vector (row stride 2208), 6+3t / 7+3t = fc1 output of iteration t, 8+3t = fc2 output.
extern "C" int dyb_hmr_feature_info_ex(const void* plan, int which, int train, long long* offset, int* dims4, int* row_stride);
extern "C" int dyb_hmr_feature_info(const void* plan, int which, long long* offset, int* dims4, int* row_stride) {
  return dyb_hmr_feature_info_ex(plan, which, 0, offset, dims4, row_stride);
}
// train != 0: features 7+3t are the fc1 outputs AFTER drop1 (model/hmr.py:165-166); in eval mode Dropout is the identity and
// they alias features 6+3t
extern "C" int dyb_hmr_feature_info_ex(const void* plan, int which, int train, long long* offset, int* dims4, int* row_stride) {
  const HmrPlan* P = reinterpret_cast<const HmrPlan*>(plan);
  DYB_REQUIRE(P && offset && dims4 && row_stride && which >= 0 && which < 15, DYB_ERR_ARG);
  dims4[0] = P->B; dims4[1] = dims4[2] = dims4[3] = 0;
  if (which == 0) {
    const ConvL& c = P->convs[0];
    *offset = (long long)c.y; dims4[1] = c.Ho; dims4[2] = c.Wo; dims4[3] = c.K; *row_stride = c.K;
  } else if (which <= 4) {
    const ConvL& c = P->convs[P->blocks[P->layer_last_block[which - 1]].c3];
    *offset = (long long)c.out; dims4[1] = c.Ho; dims4[2] = c.Wo; dims4[3] = c.K; *row_stride = c.K;
  } else if (which == 5) {
    *offset = (long long)P->a_xc[0]; dims4[1] = FEAT; *row_stride = FC1_IN_PAD;
  } else {
    int t = (which - 6) / 3, r = (which - 6) % 3;
    *offset = (long long)(r == 2 ? P->a_h2[t] : ((r == 1 && train) ? P->a_h1d[t] : P->a_h1[t])); dims4[1] = HID; *row_stride = HID;
  }
  return DYB_OK;
}
extern "C" long long dyb_hmr_act_offset_rotmat(const void* plan) { return (long long)reinterpret_cast<const HmrPlan*>(plan)->a_rot; }
extern "C" long long dyb_hmr_act_offset_state(const void* plan) { return (long long)reinterpret_cast<const HmrPlan*>(plan)->a_state; }

#define RUN(x)                  \
  do {                          \
    int rc__ = (x);             \
    if (rc__ != DYB_OK) return rc__; \
  } while (0)

// ---- nn.Dropout(p = 0.5) of the regressor (reference model/hmr.py:84,86,165,169), train mode only ------------------------
// Counter-based (Philox-4x32-10): the keep mask of element i of stream s is a pure function of (seed, offset, s, i), so
// the backward pass regenerates it instead of storing it.  y = x * keep / (1 - p).
struct DropCfg {
  int on;
  unsigned long long seed, offset;
  float p;
};
// y[i] = x[i] * keep(i) / (1 - p); y may alias x (backward: the gradient is masked in place).  n % 4 == 0.
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, float* __restrict__ y, int n4, DropCfg d,
                                                      unsigned stream_id, DybRep R) {
  DYB_REP_PROLOGUE(R);
  DYB_RB(R, x); DYB_RB(R, y);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  unsigned r[4];
  philox4x32_10((unsigned)i, stream_id, (unsigned)d.offset, (unsigned)(d.offset >> 32) + (unsigned)dyb_rep * 0x632BE5ABu,
                (unsigned)d.seed, (unsigned)(d.seed >> 32), r);
  const float scale = 1.f / (1.f - d.p);
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  float4 o;
  // uniform in [0, 1) from the top 24 bits; keep with probability 1 - p
  o.x = ((r[0] >> 8) * (1.f / 16777216.f) >= d.p) ? v.x * scale : 0.f;
  o.y = ((r[1] >> 8) * (1.f / 16777216.f) >= d.p) ? v.y * scale : 0.f;
  o.z = ((r[2] >> 8) * (1.f / 16777216.f) >= d.p) ? v.z * scale : 0.f;
  o.w = ((r[3] >> 8) * (1.f / 16777216.f) >= d.p) ? v.w * scale : 0.f;
  reinterpret_cast<float4*>(y)[i] = o;
}
static int dropout_launch(const float* x, float* y, int n, const DropCfg& d, unsigned stream_id, hipStream_t st) {
  DYB_REQUIRE(n % 4 == 0, DYB_ERR_UNSUPPORTED);
  const DybRep& R = dyb_rep_current();
  hipLaunchKernelGGL(dropout_kernel, dim3(dyb_cdiv(n / 4, 256), 1, R.n), dim3(256), 0, st, x, y, n / 4, d, stream_id, R);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
static const DropCfg kNoDrop = {0, 0, 0, 0.f};

struct WsCarve {
  char *conv, *conv_aux, *lin;
  float* gn[3];                // forward GroupNorm partials: two alternating slots for the main branch, one for the shortcut
  float* gnb;
  float* g[3];
  float* dy;
  float* reg;
  float* dy2;
  unsigned* sync;
};
static WsCarve carve(const HmrPlan& P, void* ws) {
  WsCarve c;
  char* b = reinterpret_cast<char*>(ws);
  c.conv = b; b += P.ws_conv;
  c.conv_aux = b; b += P.ws_conv_aux;
  for (int i = 0; i < 3; ++i) { c.gn[i] = reinterpret_cast<float*>(b); b += P.ws_gn; }
  c.gnb = reinterpret_cast<float*>(b); b += P.ws_gnb;
  c.lin = b; b += P.ws_lin;
  for (int i = 0; i < 3; ++i) { c.g[i] = reinterpret_cast<float*>(b); b += P.ws_grad_each; }
  c.dy = reinterpret_cast<float*>(b); b += P.ws_dy;
  c.reg = reinterpret_cast<float*>(b); b += P.ws_reg;
  c.dy2 = reinterpret_cast<float*>(b); b += P.ws_dy2;
  c.sync = reinterpret_cast<unsigned*>(b);
  return c;
}

// counter region `which` (0: the chain's stream, 1: the auxiliary stream) of the in-kernel split-K fold (igemm_conv.hip)
static unsigned* conv_ctr(const HmrPlan& P, const WsCarve& w, int which) {
  return w.sync + align64(P.convs.size() * SYNC_WORDS) + (size_t)which * DYB_CONV_SYNC_WORDS;
}
// one forward layer: conv (+ the producer's GroupNorm/ReLU applied in its loader when `prev` is given) and the
// GroupNorm statistics of its raw output into `part_out` (*nch_out partial records)
static int conv_stats(const HmrPlan& P, const ConvL& c, const float* params, float* acts, const float* x, const ConvL* prev,
                      const float* part_prev, int nch_prev, float* part_out, int* nch_out, const WsCarve& w, hipStream_t st) {
  if (prev)
    return dyb_conv2d_nhwc_fwd_gnstats(acts + prev->y, part_prev, nch_prev, params + prev->gam, params + prev->bet, 1,
                                       acts + prev->stats, params + c.w, acts + c.y, part_out, nch_out, P.B, c.H, c.W, c.C, c.K,
                                       c.R, c.S, c.stride, c.pad, w.conv, P.ws_conv, st);
  return dyb_conv2d_nhwc_fwd_gnstats(x, nullptr, 0, nullptr, nullptr, 0, nullptr, params + c.w, acts + c.y, part_out, nch_out,
                                     P.B, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad, w.conv, P.ws_conv, st);
}

// bf16-MFMA variant (BASELINE configs[4]): master weights, activations, GroupNorm statistics and accumulators stay fp32; the
// conv operand tiles are rounded to bf16 as they are staged for v_mfma_f32_32x32x16_bf16.  Per plan; default off (the parity
// mode is fp32).
extern "C" int dyb_hmr_set_bf16(void* plan, int on) {
  HmrPlan* P = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(P, DYB_ERR_ARG);
  P->bf16 = on ? 1 : 0;
  return DYB_OK;
}
extern "C" int dyb_hmr_set_graph_mode(void* plan, int on) {
  HmrPlan* P = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(P, DYB_ERR_ARG);
  P->graph_mode = on ? 1 : 0;
  return DYB_OK;
}
// stats[0..9] = graph replays, eager calls, captures, distinct forward keys, distinct backward keys,
// capture failures at: begin, body, end, instantiate, first launch
extern "C" int dyb_hmr_graph_stats(const void* plan, long long* stats10) {
  const HmrPlan* P = reinterpret_cast<const HmrPlan*>(plan);
  DYB_REQUIRE(P && stats10, DYB_ERR_ARG);
  stats10[0] = P->g_hits; stats10[1] = P->g_eager; stats10[2] = P->g_captures;
  stats10[3] = (long long)P->gfwd.size(); stats10[4] = (long long)P->gbwd.size();
  stats10[5] = P->g_fail_begin; stats10[6] = P->g_fail_body; stats10[7] = P->g_fail_end; stats10[8] = P->g_fail_inst;
  stats10[9] = P->g_fail_launch;
  return DYB_OK;
}

// Run `body` either eagerly, or - in graph mode - through the cache: a key seen for the second time
// is captured on `st` (thread-local capture; the body only enqueues kernels / D2D copies / event
// fork-joins with the auxiliary stream) and from then on replayed.  Any capture failure marks the
// key bad and falls back to eager execution, so results never depend on the graph path.
template <class Body>
static int run_cached(HmrPlan& P, std::unordered_map<GKey, GEntry, GKeyHash>& cache, const GKey& key, hipStream_t st,
                      Body body) {
  if (!P.graph_mode) return body();
  // graph mode: lookups, insertions (which may rehash) and the counters are serialised; a capture is thread-local, so
  // holding the lock across it only delays other graph-mode callers of the same plan.  The cache stops growing at
  // DYB_MAX_GRAPHS keys: later keys run eagerly.
  std::lock_guard<std::mutex> lock(P.mu);
  if (cache.find(key) == cache.end() && cache.size() >= DYB_MAX_GRAPHS) { ++P.g_eager; return body(); }
  GEntry& e = cache[key];
  if (e.exec) {
    if (hipGraphLaunch(e.exec, st) == hipSuccess) { ++P.g_hits; return DYB_OK; }
    e.bad = true;
    (void)hipGraphExecDestroy(e.exec);
    e.exec = nullptr;
  }
  ++e.seen;
  if (!e.bad && e.seen >= 2 && P.g_captures < DYB_MAX_GRAPHS) {
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
      int rc = body();
      hipGraph_t graph = nullptr;
      hipError_t er = hipStreamEndCapture(st, &graph);
      if (rc != DYB_OK) ++P.g_fail_body;
      else if (er != hipSuccess || !graph) ++P.g_fail_end;
      if (rc == DYB_OK && er == hipSuccess && graph) {
        hipGraphExec_t exec = nullptr;
        if (hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess && exec) {
          (void)hipGraphDestroy(graph);
          ++P.g_captures;
          e.exec = exec;
          if (hipGraphLaunch(exec, st) == hipSuccess) { ++P.g_hits; return DYB_OK; }
          ++P.g_fail_launch;
          e.bad = true;
          return DYB_ERR_LAUNCH;
        }
        ++P.g_fail_inst;
      }
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      e.bad = true;                 // nothing ran (capture only records): fall through to eager
    } else {
      ++P.g_fail_begin;
      (void)hipGetLastError();
      e.bad = true;
    }
  }
  ++P.g_eager;
  return body();
}

// image: [B][3][H][W] fp32 (NCHW, as the reference's dataloader produces it); init_state:
// [B][160] = init_pose | init_shape | init_cam | 0.  Results land in the activation arena.
static int forward_body(const HmrPlan& P, const float* params, const float* init_state, int n_iter, float* acts,
                        const WsCarve& w, hipStream_t st, const DropCfg& drop = kNoDrop, const DybFwdGates* gates = nullptr);

extern "C" int dyb_hmr_forward(void* plan, const float* params, const float* image, const float* init_state,
                               int n_iter, float* acts, void* ws, size_t ws_bytes, hipStream_t st) {
  HmrPlan* Pp = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(Pp && params && image && init_state && acts && ws, DYB_ERR_ARG);
  DYB_REQUIRE(n_iter >= 1 && n_iter <= MAX_ITER, DYB_ERR_UNSUPPORTED);
  HmrPlan& P = *Pp;
  DYB_REQUIRE(ws_bytes >= P.ws_total, DYB_ERR_WORKSPACE);
  DYB_REQUIRE(P.featHW == 49, DYB_ERR_UNSUPPORTED);        // AvgPool2d(7) on a 7x7 map
  WsCarve w = carve(P, ws);
  // the image pointer changes every frame: its repack stays outside the cached graph
  RUN(dyb_nchw3_to_nhwc4(image, acts + P.a_x4, P.B, P.H, P.W, st));
  GKey key{{(uintptr_t)params, (uintptr_t)init_state, (uintptr_t)acts, (uintptr_t)ws, (uintptr_t)st, (uintptr_t)n_iter, 0, 0, 0, 0}};
  return run_cached(P, P.gfwd, key, st, [&]() { return forward_body(P, params, init_state, n_iter, acts, w, st); });
}

static int forward_body(const HmrPlan& P, const float* params, const float* init_state, int n_iter, float* acts,
                        const WsCarve& w, hipStream_t st, const DropCfg& drop, const DybFwdGates* gates) {
  DybBf16Scope bf(P.bf16 != 0);
  const int B = P.B;
  const ConvL& stem = P.convs[0];
  // split-K folds happen inside the conv launches, on this pass's counters (zero before the first launch; every launch leaves them zero)
  RUN(dyb_zero_words(conv_ctr(P, w, 0), DYB_CONV_SYNC_WORDS, st));
  DybConvSyncScope conv_sync(conv_ctr(P, w, 0), DYB_CONV_SYNC_WORDS);
  int nA = 0, nB = 0, nD = 0;                 // partial counts behind w.gn[0], [1], [2]
  RUN(conv_stats(P, stem, params, acts, acts + P.a_x4, nullptr, nullptr, 0, w.gn[0], &nA, w, st));
  RUN(dyb_groupnorm_apply_n(acts + stem.y, w.gn[0], nA, params + stem.gam, params + stem.bet, nullptr, nullptr, 0, nullptr,
                            nullptr, nullptr, acts + stem.out, acts + stem.stats, B, stem.Ho * stem.Wo, stem.K, 1, st));
  RUN(dyb_maxpool3x3s2_fwd(acts + stem.out, acts + P.a_pool, reinterpret_cast<uint32_t*>(acts + P.a_poolidx), B, stem.Ho,
                           stem.Wo, stem.K, st));
  const float* x = acts + P.a_pool;
  for (int bi = 0; bi < (int)P.blocks.size(); ++bi) {
    const BlockL& b = P.blocks[bi];
    const ConvL &c1 = P.convs[b.c1], &c2 = P.convs[b.c2], &c3 = P.convs[b.c3];
    if (gates) {                   // weights updated by arena ranges on another stream: wait right before a range's first reader
      if (bi == P.layer_last_block[1] + 1) {
        if (gates->ev[0] && hipStreamWaitEvent(st, gates->ev[0], 0) != hipSuccess) return DYB_ERR_LAUNCH;
        if (gates->late) {           // the forward has reached layer3: the caller's deferred work may start now
          if (gates->mid && hipEventRecord(gates->mid, st) != hipSuccess) return DYB_ERR_LAUNCH;
          RUN(gates->late(gates->user));
        }
      }
      if (bi == P.layer_last_block[2] + 1) {
        if (gates->ev[1] && hipStreamWaitEvent(st, gates->ev[1], 0) != hipSuccess) return DYB_ERR_LAUNCH;
        // the previous backward's deferred layer4 weight gradients still read layer4's activations and write its weights
        if (gates->l4 && hipStreamWaitEvent(st, gates->l4, 0) != hipSuccess) return DYB_ERR_LAUNCH;
      }
    }
    // 3 launches per conv become 2 (or 1: the small 1x1 layers write their statistics themselves): bn1 / bn2 (+ReLU)
    // are applied by conv2 / conv3 while loading
    RUN(conv_stats(P, c1, params, acts, x, nullptr, nullptr, 0, w.gn[0], &nA, w, st));
    RUN(conv_stats(P, c2, params, acts, nullptr, &c1, w.gn[0], nA, w.gn[1], &nB, w, st));
    if (b.cd >= 0) RUN(conv_stats(P, P.convs[b.cd], params, acts, x, nullptr, nullptr, 0, w.gn[2], &nD, w, st));
    RUN(conv_stats(P, c3, params, acts, nullptr, &c2, w.gn[1], nB, w.gn[0], &nA, w, st));
    // out = relu(bn3(y3) + shortcut), the shortcut being x or downsample.1(yd) normalised on the fly
    if (b.cd >= 0) {
      const ConvL& cd = P.convs[b.cd];
      RUN(dyb_groupnorm_apply_n(acts + c3.y, w.gn[0], nA, params + c3.gam, params + c3.bet, acts + cd.y, w.gn[2], nD,
                                params + cd.gam, params + cd.bet, acts + cd.stats, acts + c3.out, acts + c3.stats, B,
                                c3.Ho * c3.Wo, c3.K, 1, st));
    } else {
      RUN(dyb_groupnorm_apply_n(acts + c3.y, w.gn[0], nA, params + c3.gam, params + c3.bet, x, nullptr, 0, nullptr, nullptr,
                                nullptr, acts + c3.out, acts + c3.stats, B, c3.Ho * c3.Wo, c3.K, 1, st));
    }
    x = acts + c3.out;
  }
  float* dsts[MAX_ITER];
  for (int t = 0; t < n_iter; ++t) dsts[t] = acts + P.a_xc[t];
  // (the previous backward's deferred regressor weight gradients read xc / h1 / h2 and write fc1 / fc2 / the decoder)
  if (gates && gates->reg && hipStreamWaitEvent(st, gates->reg, 0) != hipSuccess) return DYB_ERR_LAUNCH;
  RUN(dyb_avgpool_fwd_tail(x, dsts, n_iter, FC1_IN_PAD, B, P.featHW, FEAT, init_state, STATE_LD, STATE_LD, FEAT, st));
  // fc1 over xc = [pooled feature (2048) | state (157)]: the feature is the same in every iteration, so its 93 % of the weight
  // matrix is streamed ONCE per forward (pre = b + W[:, :2048] feat) and each iteration adds the state columns' product
  // (model/hmr.py:160-163; at 32 sequences fc1 is 289 MB per pass)
  float* fc1_pre = reinterpret_cast<float*>(w.lin);
  RUN(dyb_linear_fwd(acts + P.a_xc[0], FC1_IN_PAD, params + P.fc1_w, FC1_IN_PAD, params + P.fc1_b, nullptr, 0, fc1_pre, HID, B, FEAT, HID, st));
  for (int t = 0; t < n_iter; ++t) {
    const float* xc = acts + P.a_xc[t];
    RUN(dyb_linear_fwd(xc + FEAT, FC1_IN_PAD, params + P.fc1_w + FEAT, FC1_IN_PAD, nullptr, fc1_pre, HID, acts + P.a_h1[t], HID, B,
                       FC1_IN_PAD - FEAT, HID, st));
    // train mode: xc = drop1(fc1(xc)); xc = drop2(fc2(xc)) (model/hmr.py:163-169); eval: Dropout is the identity
    const float* h1 = acts + P.a_h1[t];
    if (drop.on) {
      RUN(dropout_launch(h1, acts + P.a_h1d[t], B * HID, drop, 2u * t, st));
      h1 = acts + P.a_h1d[t];
    }
    RUN(dyb_linear_fwd(h1, HID, params + P.fc2_w, HID, params + P.fc2_b, nullptr, 0, acts + P.a_h2[t], HID, B, HID, HID, st));
    const float* h2 = acts + P.a_h2[t];
    if (drop.on) {
      RUN(dropout_launch(h2, acts + P.a_h2d[t], B * HID, drop, 2u * t + 1u, st));
      h2 = acts + P.a_h2d[t];
    }
    float* nxt = (t + 1 < n_iter) ? acts + P.a_xc[t + 1] + FEAT : acts + P.a_state;
    int ldn = (t + 1 < n_iter) ? FC1_IN_PAD : STATE_LD;
    RUN(dyb_linear_fwd(h2, HID, params + P.dec_w, HID, params + P.dec_b, xc + FEAT, FC1_IN_PAD, nxt, ldn, B, HID, STATE_LD, st));
  }
  RUN(dyb_rot6d_fwd(acts + P.a_state, STATE_LD, acts + P.a_rot, B, st));
  return DYB_OK;
}

// A gradient tensor that may still be spread over the split-K slabs of the data-gradient convolution
// that produced it (plus an addend, the residual-edge gradient): the next GroupNorm-backward reduce
// folds it while it reads it, which removes the stand-alone fold launch from the critical chain.
struct Pending {
  const float* base;
  int nslabs;
  size_t stride;
  const float* addend;
};
static Pending plain(const float* p) { return Pending{p, 1, 0, nullptr}; }

// GroupNorm backward of layer ci, reduce half only: dm = din masked by the layer's ReLU lands in the
// layer's own slot of the dm arena (relu == 0 and din plain: dm aliases din, which then must itself be
// such a slot), the partial sums in the layer's slot of the gnb arena.  dy = rstd*(gamma*dm - c1 -
// xhat*c2) is never materialised: the data-gradient conv below and the weight-gradient conv form it in
// their operand loaders.  The weight gradient (which also writes dgamma / dbeta) is off the critical
// path, so it goes to the auxiliary stream when given, ordered by one event per layer, with its own
// split-K slab region; everything it reads lives in per-layer slots that nothing overwrites during the call.
struct WgradJob {
  int ci;
  const float* conv_in;
  const ConvL* in_prev;
  const float* dm;
  int nch, ncolb;              // layout of the layer's partial block (0 = gn_bwd_reduce's)
  const float* dy;             // throughput schedule: the layer's materialised dy (NULL: formed in the loader from dm)
};
// per-call bookkeeping of the backward chain: which layers' partial blocks have a non-default layout (written by a K4
// data-gradient epilogue) and which layers' reduce has already happened there
struct BwdState {
  std::vector<int> nch, ncolb;
  std::vector<char> reduced;
};
static int run_wgrad(HmrPlan& P, const WgradJob& j, const float* params, const float* acts, float* grads, const WsCarve& w,
                     void* slabs, hipStream_t st) {
  const ConvL& c = P.convs[j.ci];
  const float* part = w.gnb + c.gnb;
  const ConvL* ip = j.in_prev;       // non-null: the conv's input was relu(gn(y_prev)), never materialised
  DybConvSyncScope conv_sync(conv_ctr(P, w, slabs == (void*)w.conv_aux ? 1 : 0), DYB_CONV_SYNC_WORDS);   // auxiliary stream: its own counters
  if (j.dy) {
    ConvDesc d{P.B, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad};
    return dyb_conv_wgrad_plain(d, ip ? nullptr : j.conv_in, ip ? acts + ip->y : nullptr, ip ? acts + ip->stats : nullptr,
                                ip ? params + ip->gam : nullptr, ip ? params + ip->bet : nullptr, j.dy, grads + c.w, slabs, P.ws_conv, st);
  }
  return dyb_conv2d_nhwc_wgrad_gn_n(ip ? nullptr : j.conv_in, ip ? acts + ip->y : nullptr, ip ? acts + ip->stats : nullptr,
                                    ip ? params + ip->gam : nullptr, ip ? params + ip->bet : nullptr, j.dm, acts + c.y,
                                    acts + c.stats, part, j.nch, j.ncolb, params + c.gam, grads + c.w, grads + c.gam,
                                    grads + c.bet, P.B, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad, slabs, P.ws_conv, st);
}
// `jobs`: weight gradients whose inputs are ready once the reduce carrying `done` has run; the caller
// flushes them to the auxiliary stream once per bottleneck (one cross-stream edge per block instead of
// one per layer: each edge costs ~9 us of host time).  Without an auxiliary stream they run in line.
static int layer_gn_bwd(HmrPlan& P, int ci, const float* params, const float* acts, float* grads, const float* conv_in,
                        const ConvL* in_prev, const Pending& din, int relu, const float** dm_out, const WsCarve& w,
                        hipStream_t st, std::vector<WgradJob>* jobs, hipEvent_t done, bool dm_read_later = true) {
  const ConvL& c = P.convs[ci];
  const bool alias = !relu && din.nslabs == 1 && !din.addend;
  float* dm = alias ? const_cast<float*>(din.base) : w.dy + c.dy;
  float* part = w.gnb + c.gnb;
  // ReLU mask: the saved activation where it exists, else recomputed from y (bn1 / bn2)
  const bool tp = dyb_throughput_mode(P.B);
  WgradJob j{ci, conv_in, in_prev, dm, 0, 0, nullptr};
  // throughput schedule, one image per replica: the one-pass backward (every tensor read / written once: norm_pool.hip)
  int kop = 0;
  if (tp && dyb_switch(DYB_SW_tp_gn_onepass) > 0) {
    kop = dyb_gn_onepass_chunks(P.B, c.Ho * c.Wo, c.K, dyb_switch(DYB_SW_tp_gn_cap));
    if (kop > 1 && (dyb_switch(DYB_SW_tp_gn_onepass) < 2 || dyb_gn_onepass_part_floats(kop, c.K) > dyb_groupnorm_bwd_partial_floats(P.B, c.Ho * c.Wo, c.K)))
      kop = 0;
  }
  if (kop > 0) {
    float* dyl = w.dy2 + c.dy;
    RUN(dyb_gn_bwd_onepass(din.base, din.nslabs, din.stride, din.addend, c.has_out ? acts + c.out : nullptr, acts + c.y, acts + c.stats,
                           params + c.gam, params + c.bet, (alias || !dm_read_later) ? nullptr : dm, dyl, grads + c.gam, grads + c.bet,
                           c.Ho * c.Wo, c.K, relu, kop, part, w.sync + (size_t)ci * SYNC_WORDS, st));
    if (done && hipEventRecord(done, st) != hipSuccess) return DYB_ERR_LAUNCH;
    j.dy = dyl;
    if (jobs) jobs->push_back(j);
    else RUN(run_wgrad(P, j, params, acts, grads, w, w.conv, st));
    *dm_out = dm;
    return DYB_OK;
  }
  RUN(dyb_gn_bwd_reduce_slabs(din.base, din.nslabs, din.stride, din.addend, c.has_out ? acts + c.out : nullptr, acts + c.y,
                              acts + c.stats, params + c.gam, params + c.bet, dm, part, P.B, c.Ho * c.Wo, c.K, relu, st,
                              tp ? nullptr : done));
  if (tp) {
    // throughput schedule: dy once per layer (also dgamma / dbeta), plain gradient convolutions afterwards
    float* dyl = w.dy2 + c.dy;
    RUN(dyb_gn_bwd_apply_dy(dm, acts + c.y, acts + c.stats, part, 0, 0, params + c.gam, dyl, grads + c.gam, grads + c.bet, P.B,
                            c.Ho * c.Wo, c.K, st));
    if (done && hipEventRecord(done, st) != hipSuccess) return DYB_ERR_LAUNCH;
    j.dy = dyl;
  }
  if (jobs) jobs->push_back(j);
  else RUN(run_wgrad(P, j, params, acts, grads, w, w.conv, st));
  *dm_out = dm;
  return DYB_OK;
}
// (`held`: jobs of `deferrable` layers in the throughput form are kept for the end of the call instead)
static int flush_wgrads(HmrPlan& P, std::vector<WgradJob>& jobs, hipEvent_t done, const float* params, const float* acts,
                        float* grads, const WsCarve& w, hipStream_t aux, const std::vector<char>& deferrable,
                        std::vector<WgradJob>& held) {
  if (hipStreamWaitEvent(aux, done, 0) != hipSuccess) return DYB_ERR_LAUNCH;
  for (const WgradJob& j : jobs) {
    if (deferrable[j.ci] && j.dy) held.push_back(j);
    else RUN(run_wgrad(P, j, params, acts, grads, w, w.conv_aux, aux));
  }
  jobs.clear();
  return DYB_OK;
}
// data gradient of layer ci from its dm: conv_transpose(dy, w) (+ addend), materialised in dx_buf or -
// when `out` is given and the policy splits K - left as slabs (+ the addend) for the next reduce
static int layer_dgrad(HmrPlan& P, int ci, const float* params, const float* acts, const float* dm, float* dx_buf,
                       const float* addend, Pending* out, const WsCarve& w, hipStream_t st, const BwdState& bs) {
  const ConvL& c = P.convs[ci];
  ConvDesc d{P.B, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad};
  GnBwdSrc src{dm, acts + c.y, acts + c.stats, w.gnb + c.gnb, params + c.gam, bs.nch[ci], bs.ncolb[ci]};
  int ns = 1;
  if (dyb_throughput_mode(P.B))    // dy of this layer was materialised by its reduce step (layer_gn_bwd)
    RUN(dyb_conv_dgrad_plain_raw(d, w.dy2 + c.dy, params + c.w, dx_buf, addend, w.conv, P.ws_conv,
                                 (out && P.fold_in_reduce) ? &ns : nullptr, st));
  else
    RUN(dyb_conv_dgrad_gn_raw(d, src, params + c.w, dx_buf, addend, w.conv, P.ws_conv, (out && P.fold_in_reduce) ? &ns : nullptr,
                              st));
  if (out) {
    if (ns > 1) *out = Pending{reinterpret_cast<const float*>(w.conv), ns, (size_t)P.B * c.H * c.W * c.C, addend};
    else *out = plain(dx_buf);
  }
  return DYB_OK;
}

// K4 data gradient of the 1x1 layer ci whose epilogue performs the GroupNorm-backward reduce of the producer layer pi
// (the layer whose normalised output is ci's input): dm_pi + partial block of pi come out, no dx buffer exists.
// Returns false in *done when the shape does not qualify (caller takes the two-launch route).
static int layer_dgrad_k4(HmrPlan& P, int ci, int pi, const float* params, const float* acts, const float* dm, const float* addend,
                          const WsCarve& w, hipStream_t st, BwdState& bs, const float** dm_p, bool* done) {
  const ConvL &c = P.convs[ci], &p = P.convs[pi];
  ConvDesc d{P.B, c.H, c.W, c.C, c.K, c.R, c.S, c.stride, c.pad};
  *done = false;
  if (!dyb_conv_dgrad_k4_ok(d)) return DYB_OK;
  GnBwdSrc src{dm, acts + c.y, acts + c.stats, w.gnb + c.gnb, params + c.gam, bs.nch[ci], bs.ncolb[ci]};
  int nch = 0, ncolb = 0;
  RUN(dyb_conv_dgrad_k4(d, src, params + c.w, addend, acts + p.y, p.has_out ? acts + p.out : nullptr, acts + p.stats,
                        params + p.gam, params + p.bet, w.dy + p.dy, w.gnb + p.gnb, &nch, &ncolb, st, nullptr));
  bs.nch[pi] = nch; bs.ncolb[pi] = ncolb; bs.reduced[pi] = 1;
  *dm_p = w.dy + p.dy;
  *done = true;
  return DYB_OK;
}

// d_rotmat: [B][24][9]; d_state: [B][160], only columns 144..156 (shape, cam) are read.
// grads: parameter-arena-shaped buffer, every tensor's span is overwritten (pad gaps untouched:
// zero them once at allocation).
// aux_stream (may be NULL): a second stream the weight-gradient convolutions are issued on; the call
// returns with `stream` already waiting for them, so callers keep ordering on `stream` only.
static int backward_body(HmrPlan& P, const float* params, const float* acts, const float* d_rotmat, const float* d_state,
                         int n_iter, float* grads, const WsCarve& w, hipStream_t st, hipStream_t aux, const DybEvents& E,
                         const DropCfg& drop = kNoDrop, bool defer_req = false, int* n_deferred = nullptr);

// the same call with the caller's own event set and no graph cache: what the native frame stepper issues (several chains
// of one plan may be in flight on different streams, each with its own workspace and events)
int dyb_hmr_backward_ev(void* plan, const float* params, const float* acts, const float* d_rotmat, const float* d_state,
                        int n_iter, float* grads, void* ws, size_t ws_bytes, hipStream_t st, hipStream_t aux, const DybEvents* ev,
                        bool defer, int* n_deferred) {
  HmrPlan* Pp = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(Pp && params && acts && d_rotmat && d_state && grads && ws, DYB_ERR_ARG);
  DYB_REQUIRE(n_iter >= 1 && n_iter <= MAX_ITER, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(ws_bytes >= Pp->ws_total, DYB_ERR_WORKSPACE);
  if (aux == st || !ev) aux = nullptr;
  WsCarve w = carve(*Pp, ws);
  static const DybEvents none;
  return backward_body(*Pp, params, acts, d_rotmat, d_state, n_iter, grads, w, st, aux, ev ? *ev : none, kNoDrop, defer, n_deferred);
}
// forward without the graph cache (same reason)
void dyb_hmr_param_groups(const void* plan, size_t bounds[2]) {
  const HmrPlan* P = reinterpret_cast<const HmrPlan*>(plan);
  bounds[0] = P->convs[P->blocks[P->layer_last_block[1] + 1].c1].w;       // first tensor of layer3
  bounds[1] = P->convs[P->blocks[P->layer_last_block[2] + 1].c1].w;       // first tensor of layer4 (the regressor follows)
}
int dyb_hmr_forward_plain(void* plan, const float* params, const float* image, const float* init_state, int n_iter, float* acts,
                          void* ws, size_t ws_bytes, hipStream_t st, const DybFwdGates* gates) {
  HmrPlan* Pp = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(Pp && params && image && init_state && acts && ws, DYB_ERR_ARG);
  DYB_REQUIRE(n_iter >= 1 && n_iter <= MAX_ITER, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(ws_bytes >= Pp->ws_total && Pp->featHW == 49, DYB_ERR_WORKSPACE);
  WsCarve w = carve(*Pp, ws);
  RUN(dyb_nchw3_to_nhwc4(image, acts + Pp->a_x4, Pp->B, Pp->H, Pp->W, st));
  return forward_body(*Pp, params, init_state, n_iter, acts, w, st, kNoDrop, gates);
}

// train-mode variants: nn.Dropout(0.5) after fc1 / fc2 of every regressor iteration (reference model/hmr.py:84,86,165,169).
// (seed, offset) select the masks; the backward of a forward must be given the same pair.  No graph cache.
extern "C" int dyb_hmr_forward_train(void* plan, const float* params, const float* image, const float* init_state, int n_iter,
                                     float* acts, void* ws, size_t ws_bytes, unsigned long long seed, unsigned long long offset,
                                     float p, hipStream_t st) {
  HmrPlan* Pp = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(Pp && params && image && init_state && acts && ws && p >= 0.f && p < 1.f, DYB_ERR_ARG);
  DYB_REQUIRE(n_iter >= 1 && n_iter <= MAX_ITER, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(ws_bytes >= Pp->ws_total && Pp->featHW == 49, DYB_ERR_WORKSPACE);
  WsCarve w = carve(*Pp, ws);
  RUN(dyb_nchw3_to_nhwc4(image, acts + Pp->a_x4, Pp->B, Pp->H, Pp->W, st));
  const DropCfg d{1, seed, offset, p};
  return forward_body(*Pp, params, init_state, n_iter, acts, w, st, d);
}
extern "C" int dyb_hmr_backward_train(void* plan, const float* params, const float* acts, const float* d_rotmat,
                                      const float* d_state, int n_iter, float* grads, void* ws, size_t ws_bytes,
                                      unsigned long long seed, unsigned long long offset, float p, hipStream_t st, hipStream_t aux) {
  HmrPlan* Pp = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(Pp && params && acts && d_rotmat && d_state && grads && ws && p >= 0.f && p < 1.f, DYB_ERR_ARG);
  DYB_REQUIRE(n_iter >= 1 && n_iter <= MAX_ITER, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(ws_bytes >= Pp->ws_total, DYB_ERR_WORKSPACE);
  if (aux == st) aux = nullptr;
  if (aux) RUN(ensure_events(*Pp));
  WsCarve w = carve(*Pp, ws);
  const DropCfg d{1, seed, offset, p};
  return backward_body(*Pp, params, acts, d_rotmat, d_state, n_iter, grads, w, st, aux, Pp->ev, d);
}

extern "C" int dyb_hmr_backward(void* plan, const float* params, const float* acts, const float* d_rotmat,
                                const float* d_state, int n_iter, float* grads, void* ws, size_t ws_bytes,
                                hipStream_t st, hipStream_t aux) {
  HmrPlan* Pp = reinterpret_cast<HmrPlan*>(plan);
  DYB_REQUIRE(Pp && params && acts && d_rotmat && d_state && grads && ws, DYB_ERR_ARG);
  DYB_REQUIRE(n_iter >= 1 && n_iter <= MAX_ITER, DYB_ERR_UNSUPPORTED);
  HmrPlan& P = *Pp;
  DYB_REQUIRE(ws_bytes >= P.ws_total, DYB_ERR_WORKSPACE);
  if (aux == st) aux = nullptr;
  if (aux) RUN(ensure_events(P));
  WsCarve w = carve(P, ws);
  GKey key{{(uintptr_t)params, (uintptr_t)acts, (uintptr_t)d_rotmat, (uintptr_t)d_state, (uintptr_t)grads, (uintptr_t)ws,
            (uintptr_t)st, (uintptr_t)aux, (uintptr_t)n_iter, 0}};
  return run_cached(P, P.gbwd, key, st,
                    [&]() { return backward_body(P, params, acts, d_rotmat, d_state, n_iter, grads, w, st, aux, P.ev); });
}

static int backward_body(HmrPlan& P, const float* params, const float* acts, const float* d_rotmat, const float* d_state,
                         int n_iter, float* grads, const WsCarve& w, hipStream_t st, hipStream_t aux, const DybEvents& E,
                         const DropCfg& drop, bool defer_req, int* n_deferred) {
  DybBf16Scope bf(P.bf16 != 0);
  const int B = P.B;
  float* d_st[MAX_ITER + 1];
  float *d_h2[MAX_ITER], *d_h1[MAX_ITER];
  float* r = w.reg;
  for (int t = 0; t <= MAX_ITER; ++t) { d_st[t] = r; r += (size_t)B * STATE_LD; }
  for (int t = 0; t < MAX_ITER; ++t) { d_h2[t] = r; r += (size_t)B * HID; }
  for (int t = 0; t < MAX_ITER; ++t) { d_h1[t] = r; r += (size_t)B * HID; }
  float* d_xf = r;                                         // [B][2208], columns < 2048 used

  // ---- regressor
  // (a kernel rather than a device-to-device memcpy: it is replica-aware like everything else on the chain, dyb_common.h)
  RUN(dyb_scale_add(nullptr, d_state, nullptr, d_st[n_iter], (size_t)B * STATE_LD, st));
  RUN(dyb_rot6d_bwd(acts + P.a_state, STATE_LD, d_rotmat, d_st[n_iter], STATE_LD, B, st));
  for (int t = n_iter - 1; t >= 0; --t) {
    RUN(dyb_linear_bwd_dx(d_st[t + 1], STATE_LD, params + P.dec_w, HID, B, HID, STATE_LD, d_h2[t], HID, 0, HID, nullptr, 0,
                          nullptr, 0, w.lin, P.ws_lin, st));
    if (drop.on) RUN(dropout_launch(d_h2[t], d_h2[t], B * HID, drop, 2u * t + 1u, st));       // through drop2: same mask, same scale
    RUN(dyb_linear_bwd_dx(d_h2[t], HID, params + P.fc2_w, HID, B, HID, HID, d_h1[t], HID, 0, HID, nullptr, 0, nullptr, 0,
                          w.lin, P.ws_lin, st));
    if (drop.on) RUN(dropout_launch(d_h1[t], d_h1[t], B * HID, drop, 2u * t, st));            // through drop1
    // through fc1: the state columns per iteration (d_st[t] = W[:, 2048:]^T d_h1[t] + d_st[t + 1]); the feature columns once, below
    RUN(dyb_linear_bwd_dx(d_h1[t], HID, params + P.fc1_w + FEAT, FC1_IN_PAD, B, FC1_IN_PAD - FEAT, HID, d_st[t], STATE_LD, 0, 0, d_st[t],
                          STATE_LD, d_st[t + 1], STATE_LD, w.lin, P.ws_lin, st));
  }
  {
    // d_xf = W[:, :2048]^T (sum_t d_h1[t]): one pass over the feature columns instead of one per iteration
    float* sbuf[2] = {d_xf + (size_t)B * FC1_IN_PAD, d_xf + (size_t)B * (FC1_IN_PAD + HID)};     // two [B][1024] behind d_xf in the regressor scratch
    const float* dsum = d_h1[0];
    for (int t = 1; t < n_iter; ++t) {                       // (ping-pong: the add kernel's operands may not alias its result)
      float* o = sbuf[t & 1];
      RUN(dyb_scale_add(nullptr, dsum, d_h1[t], o, (size_t)B * HID, st));
      dsum = o;
    }
    RUN(dyb_linear_bwd_dx(dsum, HID, params + P.fc1_w, FC1_IN_PAD, B, FEAT, HID, d_xf, FC1_IN_PAD, 0, FEAT, nullptr, 0, nullptr, 0, w.lin,
                          P.ws_lin, st));
  }
  // the regressor's weight gradients (fc1 / fc2 / decoder, the scope's weight update in their epilogue): HBM streams that depend on
  // nothing in the backbone backward - in line here, or with the deferred set at the end of the call
  auto regressor_dw = [&](hipStream_t s) -> int {
    const float *dys[MAX_ITER], *xs[MAX_ITER];
    int ldd[MAX_ITER], ldx[MAX_ITER];
    for (int t = 0; t < n_iter; ++t) { dys[t] = d_st[t + 1]; ldd[t] = STATE_LD; xs[t] = acts + (drop.on ? P.a_h2d[t] : P.a_h2[t]); ldx[t] = HID; }
    RUN(dyb_linear_bwd_dw(dys, ldd, xs, ldx, n_iter, B, HID, STATE_LD, grads + P.dec_w, HID, grads + P.dec_b, s));
    for (int t = 0; t < n_iter; ++t) { dys[t] = d_h2[t]; ldd[t] = HID; xs[t] = acts + (drop.on ? P.a_h1d[t] : P.a_h1[t]); ldx[t] = HID; }
    RUN(dyb_linear_bwd_dw(dys, ldd, xs, ldx, n_iter, B, HID, HID, grads + P.fc2_w, HID, grads + P.fc2_b, s));
    for (int t = 0; t < n_iter; ++t) { dys[t] = d_h1[t]; ldd[t] = HID; xs[t] = acts + P.a_xc[t]; ldx[t] = FC1_IN_PAD; }
    return dyb_linear_bwd_dw(dys, ldd, xs, ldx, n_iter, B, FC1_IN_PAD, HID, grads + P.fc1_w, FC1_IN_PAD, grads + P.fc1_b, s);
  };
  // Deferred weight gradients (`defer_req`; DybEvents, dyb_common.h): the layers whose EVERY input the next forward rewrites only behind its
  // layer4 gate - layer4's convolutions except block 0's conv1 / downsample (those two read layer3's last output, which the next
  // forward rewrites before it reaches the gate: they stay in the backward rather than pulling the forward's wait up in front of
  // layer3's last GroupNorm apply, where it would stall the forward on the whole auxiliary queue) - and the regressor.  Only the
  // throughput form qualifies (the layer's dy materialised in its own w.dy2 slot); a forward touches neither w.dy2, w.reg, the
  // auxiliary slab region nor the auxiliary counter region.
  const bool defer = aux && defer_req && E.l4 && E.reg && !drop.on;
  std::vector<char> deferrable(P.convs.size(), 0);
  if (defer) {
    const int first4 = P.layer_last_block[2] + 1;
    for (int bi = first4; bi < (int)P.blocks.size(); ++bi) {
      const BlockL& b = P.blocks[bi];
      deferrable[b.c2] = deferrable[b.c3] = 1;
      if (bi > first4) deferrable[b.c1] = 1;
    }
  }
  std::vector<WgradJob> deferred;
  if (!defer) RUN(regressor_dw(st));

  // ---- backbone, last block first.  D0/D1 ping-pong the data gradients travelling down the main
  // branch, Rb holds the shortcut branch's data gradient; the residual-edge gradient of a block is the
  // dm of its third GroupNorm (the ReLU-masked incoming gradient), used in place.
  float *D0 = w.g[0], *D1 = w.g[1], *Rb = w.g[2];
  // arrival counters of the one-pass GroupNorm backward and of the convolutions' in-kernel split-K fold (both streams' regions: the
  // auxiliary stream's launches of this call are ordered behind this point by the per-layer events)
  RUN(dyb_zero_words(w.sync, (int)(align64(P.convs.size() * SYNC_WORDS) + 2 * DYB_CONV_SYNC_WORDS), st));
  DybConvSyncScope conv_sync(conv_ctr(P, w, 0), DYB_CONV_SYNC_WORDS);
  RUN(dyb_avgpool_bwd(d_xf, FC1_IN_PAD, D0, B, P.featHW, FEAT, st));
  Pending cur = plain(D0);
  float* free_buf = D1;          // the D buffer `cur` does not occupy (a pending `cur` lives in the slab region)
  std::vector<WgradJob> jobs_store;
  std::vector<WgradJob>* jobs = aux ? &jobs_store : nullptr;
  BwdState bs;
  bs.nch.assign(P.convs.size(), 0); bs.ncolb.assign(P.convs.size(), 0); bs.reduced.assign(P.convs.size(), 0);
  // weight-gradient job of a layer whose reduce happened inside a K4 data gradient
  auto push_wgrad = [&](int ci, const float* conv_in, const ConvL* in_prev, const float* dm) -> int {
    WgradJob j{ci, conv_in, in_prev, dm, bs.nch[ci], bs.ncolb[ci], nullptr};
    if (jobs) { jobs->push_back(j); return DYB_OK; }
    return run_wgrad(P, j, params, acts, grads, w, w.conv, st);
  };
  for (int bi = (int)P.blocks.size() - 1; bi >= 0; --bi) {
    const BlockL& b = P.blocks[bi];
    const ConvL &c1 = P.convs[b.c1], &c2 = P.convs[b.c2];
    const float* xin = (bi == 0) ? acts + P.a_pool : acts + P.convs[P.blocks[bi - 1].c3].out;
    float* other = (free_buf == D0) ? D1 : D0;
    const float *dm3 = nullptr, *dm2 = nullptr, *dm1 = nullptr, *dmd = nullptr;
    Pending p3, p2, pout;
    bool k4 = false;
    hipEvent_t ev = aux ? E.dy[b.c1] : nullptr;      // rides on the block's last reduce
    // out = relu(gn3(conv3(a2)) + res)
    if (bs.reduced[b.c3]) {            // done by the K4 data gradient of the next block's conv1
      dm3 = w.dy + P.convs[b.c3].dy;
      RUN(push_wgrad(b.c3, nullptr, &c2, dm3));
    } else {
      RUN(layer_gn_bwd(P, b.c3, params, acts, grads, nullptr, &c2, cur, 1, &dm3, w, st, jobs, nullptr));
    }
    RUN(layer_dgrad_k4(P, b.c3, b.c2, params, acts, dm3, nullptr, w, st, bs, &dm2, &k4));
    if (k4) {
      RUN(push_wgrad(b.c2, nullptr, &c1, dm2));
    } else {
      RUN(layer_dgrad(P, b.c3, params, acts, dm3, free_buf, nullptr, &p3, w, st, bs));
      RUN(layer_gn_bwd(P, b.c2, params, acts, grads, nullptr, &c1, p3, 1, &dm2, w, st, jobs, nullptr, false));
    }
    RUN(layer_dgrad(P, b.c2, params, acts, dm2, other, nullptr, &p2, w, st, bs));      // `cur` was consumed by the c3 reduce
    const float* edge = dm3;           // residual-edge gradient of this block
    if (b.cd >= 0) {
      RUN(layer_gn_bwd(P, b.c1, params, acts, grads, xin, nullptr, p2, 1, &dm1, w, st, jobs, nullptr, false));
      // shortcut branch: GroupNorm without ReLU on the residual-edge gradient; its data gradient is materialised
      RUN(layer_gn_bwd(P, b.cd, params, acts, grads, xin, nullptr, plain(dm3), 0, &dmd, w, st, jobs, ev, false));
      if (aux) RUN(flush_wgrads(P, jobs_store, ev, params, acts, grads, w, aux, deferrable, deferred));
      RUN(layer_dgrad(P, b.cd, params, acts, dmd, Rb, nullptr, nullptr, w, st, bs));
      edge = Rb;
    } else {
      RUN(layer_gn_bwd(P, b.c1, params, acts, grads, xin, nullptr, p2, 1, &dm1, w, st, jobs, ev, false));
      if (aux) RUN(flush_wgrads(P, jobs_store, ev, params, acts, grads, w, aux, deferrable, deferred));
    }
    k4 = false;
    if (bi > 0) {
      const float* dmp = nullptr;
      RUN(layer_dgrad_k4(P, b.c1, P.blocks[bi - 1].c3, params, acts, dm1, edge, w, st, bs, &dmp, &k4));
    }
    if (!k4) {
      RUN(layer_dgrad(P, b.c1, params, acts, dm1, free_buf, edge, &pout, w, st, bs));
      cur = pout;
      if (cur.nslabs == 1) free_buf = other;       // cur sits in the old free buffer
    }
  }
  // ---- stem: maxpool backward needs the gradient materialised -> GN/ReLU -> conv1 (no data gradient for the image)
  const ConvL& stem = P.convs[0];
  const float* gpool = cur.base;
  float* spare = free_buf;
  if (cur.nslabs > 1) {
    RUN(dyb_splitk_fold(cur.base, cur.nslabs, (size_t)B * P.poolH * P.poolW * stem.K, cur.addend, free_buf, st));
    gpool = free_buf;
    spare = (free_buf == D0) ? D1 : D0;
  }
  RUN(dyb_maxpool3x3s2_bwd(gpool, reinterpret_cast<const uint32_t*>(acts + P.a_poolidx), spare, B, stem.Ho, stem.Wo, stem.K, st));
  const float* dm0;
  RUN(layer_gn_bwd(P, 0, params, acts, grads, acts + P.a_x4, nullptr, plain(spare), 1, &dm0, w, st, jobs,
                   aux ? E.dy[0] : nullptr, false));
  if (aux) RUN(flush_wgrads(P, jobs_store, E.dy[0], params, acts, grads, w, aux, deferrable, deferred));
  if (aux) {
    if (hipEventRecord(E.join, aux) != hipSuccess) return DYB_ERR_LAUNCH;
    if (hipStreamWaitEvent(st, E.join, 0) != hipSuccess) return DYB_ERR_LAUNCH;
    if (defer) {
      // behind the join: the chain's stream does not wait for these.  The auxiliary stream has waited for every per-block event of
      // this call (the last one, the stem's, was recorded on `st` behind the regressor's data gradients and every layer4 reduce).
      // Issued inside the call: the weight-update scope of the calling thread still holds, and its span list is complete on return.
      for (const WgradJob& j : deferred) RUN(run_wgrad(P, j, params, acts, grads, w, w.conv_aux, aux));
      if (hipEventRecord(E.l4, aux) != hipSuccess) return DYB_ERR_LAUNCH;
      RUN(regressor_dw(aux));
      if (hipEventRecord(E.reg, aux) != hipSuccess) return DYB_ERR_LAUNCH;
      if (n_deferred) *n_deferred += (int)deferred.size() + 3;
    }
  }
  return DYB_OK;
}

#include "hvp_engine.inc"
