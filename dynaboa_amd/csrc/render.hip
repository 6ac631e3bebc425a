// Mesh overlay on the device: a deterministic triangle rasteriser that draws N meshes (one per sequence of a step) over their
// frames in one call.  It stands where the reference draws one frame at a time through pyrender on OpenGL and the host
// (render_demo.py:58-134 as called from base_adaptor.py:429-443): the mesh turned 180 degrees about X, a weak-perspective
// camera (sx, sy, tx, ty), three point lights, one opaque colour, the picture pasted over the frame where the mesh covers it.
//
// Conventions (tests/render_ref.py restates them in numpy; the two agree bit for bit on coverage):
//   image position   u = W/2 (1 + sx (X + tx)),  v = H/2 (1 + sy (Y + ty))   fp32, one rounding per operation (no fused
//                    multiply-add: contraction is switched off for this file), pixel centres at (i + 0.5, j + 0.5);
//                    depth is the model's Z, smaller = nearer; no near / far plane.
//   coverage         u, v snapped to 1/256 pixel (round to nearest even), int64 edge functions, top-left fill rule: a pixel
//                    centre on an edge shared by two faces belongs to exactly one of them.  A face is drawn when its snapped
//                    area is > 0 in the orientation where the model-space normal (v1 - v0) x (v2 - v0) has negative Z (back faces
//                    and degenerate faces drop out, as for pyrender's single-sided material).  A face with a snapped coordinate
//                    beyond 2^30 (4 million pixels from the origin) or not finite, or with a corner whose Z is not finite, is
//                    dropped: inside that range the int64 edge functions (differences below 2^32, widened before they are
//                    formed, products below 2^64 / 4) cannot overflow whatever the frame size.
//   depth            (w0 z0 + w1 z1 + w2 z2) / area with the integer weights converted to fp32; nearest wins, ties go to the
//                    lower face index.  Every pixel is owned by one thread which sees every face: no atomics on the result,
//                    nothing depends on the order workgroups or threads run in.
//   shading          smooth: vertex normal = normalised sum of the unnormalised normals of the incident faces, gathered in
//                    the order of the vertex -> face CSR table (deterministic, unlike a scatter of float atomics); normal and
//                    position barycentric per pixel, normal renormalised; in the turned space p' = (X, -Y, -Z):
//                    I = min(1, 0.3 + 0.35 sum_k max(0, n' . dir(L_k - p'))), L = (0,-1,1), (0,1,1), (1,1,2), no falloff;
//                    pixel = round(255 I colour).  This is NOT pyrender's metallic-roughness shading (unpinned: pyrender is
//                    absent from the build image); geometry, visibility and the light set-up are the reference's.
//   model matrix     optional (dyb_render_opts.model, the _opt entries): one 3x3 fp32 matrix per mesh, row major, in this file's raw
//                    model space; x' = (m0 x + m1 y) + m2 z and likewise y', z', one rounding per operation.  The reference turns
//                    the mesh by Rx (180 degrees about X) and then by R(angle, axis); Rx is folded into the image coordinates here,
//                    so the matrix handed down for a side view is Rx R Rx (render.py builds it in fp64 and rounds once).  A
//                    pre-pass writes the turned vertices into the workspace and the kernels below read those rows: normals, face
//                    set-up, depth and shading see the very numbers dyb_render_transform_verts gives, so a call with a matrix
//                    equals, byte for byte, the call on vertices turned by that entry.  (-0 comes out as +0 under the identity.)
//   wireframe        optional (dyb_render_opts.wireframe): a face gives a fragment at a pixel centre iff the centre is inside it by
//                    the coverage rule above AND, for at least one of its edges e, w_e < 256 max(|dx_e|, |dy_e|) - w_e the
//                    non-negative int64 edge function of e at the centre, dx_e / dy_e the snapped extents of e widened to int64:
//                    the centre lies within one pixel of the edge along the edge's minor axis.  (256, not 128: an interior edge
//                    gets a band from each of its two faces, a silhouette edge from its one front face only.)  Nearest fragment
//                    wins, ties to the lower face index; depth and shading are the solid path's.  A pixel without a fragment keeps
//                    the frame or falls through to the mesh beneath, even where a solid face would cover it: face_id -1, depth
//                    +inf.  This follows OpenGL's line polygon mode as RenderFlags.ALL_WIREFRAME selects it - only line fragments
//                    take part in the depth test - and is unpinned like the shading (pyrender is absent from the build image).
//
// Four kernels (and the matrix pre-pass) behind the three entries (uniform: N meshes at one frame size; ragged: every mesh over a frame of its own size;
// scenes: several meshes over one frame): vertex normals (one thread per vertex), face set-up (one thread per face: snapped corners
// + pixel box, an empty box for culled / off-image faces), the pixel box of a whole mesh (one workgroup per mesh; ragged and scene
// entries), and one workgroup per 16x16 pixel tile that streams the face boxes 256 at a time, compacts the faces touching the tile
// into LDS (with their corners and depths) and lets each thread keep the nearest face of its pixel.  The list is processed chunk by
// chunk, so no per-tile capacity can overflow (the synthetic SMPL's random-triple faces put thousands of faces over one tile).
//
// The three entries are one problem at three levels of generality and run the same kernels on one table (RndTab): a ragged mesh is
// a scene of one mesh, a uniform batch a ragged call whose pointers are strided.  Between the meshes of a scene there is no depth
// test - each has a camera of its own, their Z are not comparable - but the painter rule: the mesh listed later is on top.
#include "dyb_common.h"

#pragma clang fp contract(off)

#define RND_TILE 16
#define RND_CHUNK 256
#define RND_MAX_N 64
#define RND_MAX_DIM 4096
#define RND_EMPTY_BOX 0x0000ffff                 // lo = 65535 > every pixel index, hi = 0
#define RND_SNAP_LIMIT 1073741824.0f             // 2^30 in 1/256-pixel units

typedef unsigned rnd_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int rnd_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int rnd_max(int a, int b) { return a > b ? a : b; }
static inline size_t rnd_align(size_t v) { return (v + 255) & ~(size_t)255; }

// one mesh of a ragged call (include/dynaboa_hip.h declares the same struct)
struct dyb_render_desc {
  const float* verts;
  const uint8_t* background;
  uint8_t* out;
  int H, W;
};
// one scene of a scene call (include/dynaboa_hip.h declares the same struct): meshes [mesh_begin, mesh_end) of the call's mesh list
// over one frame, in painter order
struct dyb_render_scene {
  const uint8_t* background;
  uint8_t* out;
  int* mesh_id;
  int* face_id;
  int H, W;
  int mesh_begin, mesh_end;
};
// what the _opt forms of the entries take beside the plain arguments (include/dynaboa_hip.h declares the same struct); NULL = neither
struct dyb_render_opts {
  const float* model;                     // DEVICE [meshes][9], row major; NULL: identity
  int wireframe;
};
// A call of any of the three entries as the kernels see it: scenes (a frame and the meshes [m0, m1) of the call's list over it, in
// painter order) and meshes, as kernel arguments - no allocation, no copy, no host wait.  Sizes and mesh ranges are packed so that
// 64 scenes and 64 meshes fit in the 4 KB a launch may carry (cameras and the scene entry's colours are device arrays for the same
// reason).  tile0 is the prefix of the scenes' tile counts: the flat grid of the tile kernel.
struct RndScene {
  const uint8_t* bg;
  uint8_t* out;
  int* mesh_id;
  int* face_id;
  unsigned short H, W;                    // <= RND_MAX_DIM
  unsigned char m0, m1;                   // meshes [m0, m1) of the list, <= RND_MAX_N
};
struct RndTab {
  RndScene s[RND_MAX_N];
  const float* verts[RND_MAX_N];          // per mesh
  int tile0[RND_MAX_N + 1];               // prefix of the scenes' tile counts
  unsigned char scene_of[RND_MAX_N];      // per mesh
};
// The fattest launch is the tile kernel's: the table (64 * 40 + 64 * 8 + 65 * 4 + 64 = 3396, padded to 3400), then nscenes and its
// padding (8), seven pointers (56), cr / cg / cb and V / F / use_box (24) = 3488 bytes of explicit arguments, and the 256 bytes of
// implicit arguments the runtime appends.
static_assert(sizeof(RndTab) + 8 + 56 + 24 + 256 <= 4096, "the table and the other arguments of the tile launch must fit in 4 KB");

// ---- model matrix ----------------------------------------------------------------------------------------------------------------
// o = M p, M row major: the one statement of that arithmetic (contraction is off: a product and a sum round separately)
__device__ __forceinline__ void render_xform(const float* __restrict__ m, const float* __restrict__ p, float* __restrict__ o) {
  const float x = p[0], y = p[1], z = p[2];
  o[0] = (m[0] * x + m[1] * y) + m[2] * z;
  o[1] = (m[3] * x + m[4] * y) + m[5] * z;
  o[2] = (m[6] * x + m[7] * y) + m[8] * z;
}
// the pre-pass of a call with matrices: mesh n of the table -> row n of out [M][V][3]
__global__ __launch_bounds__(256) void render_transform_tab_kernel(RndTab tab, const float* __restrict__ model, int V,
                                                                   float* __restrict__ out) {
  const int v = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
  if (v >= V) return;
  render_xform(model + 9 * n, tab.verts[n] + 3 * (size_t)v, out + ((size_t)n * V + v) * 3);
}
// the exported form: verts [N][V][3] contiguous, flat over N V; model NULL: a copy
__global__ __launch_bounds__(256) void render_transform_kernel(const float* __restrict__ verts, const float* __restrict__ model,
                                                               float* __restrict__ out, long long total, int V) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  if (model) {
    render_xform(model + 9 * (g / V), verts + 3 * g, out + 3 * g);
  } else {
    out[3 * g] = verts[3 * g];
    out[3 * g + 1] = verts[3 * g + 1];
    out[3 * g + 2] = verts[3 * g + 2];
  }
}

// ---- vertex normals ------------------------------------------------------------------------------------------------------------
// vertex v of the mesh at P -> its normal at o
__device__ __forceinline__ void render_vnormal_body(const float* __restrict__ P, const int* __restrict__ faces,
                                                    const int* __restrict__ adj_ptr, const int* __restrict__ adj_idx, int V, int F,
                                                    float* __restrict__ o, int v) {
  float sx = 0.f, sy = 0.f, sz = 0.f;
  int lo = adj_ptr[v], hi = adj_ptr[v + 1];
  lo = lo < 0 ? 0 : lo;
  hi = hi > 3 * F ? 3 * F : hi;
  for (int k = lo; k < hi; ++k) {
    const int f = adj_idx[k];
    if ((unsigned)f >= (unsigned)F) continue;
    const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) continue;
    const float ax = P[3 * i1] - P[3 * i0], ay = P[3 * i1 + 1] - P[3 * i0 + 1], az = P[3 * i1 + 2] - P[3 * i0 + 2];
    const float bx = P[3 * i2] - P[3 * i0], by = P[3 * i2 + 1] - P[3 * i0 + 1], bz = P[3 * i2 + 2] - P[3 * i0 + 2];
    sx += ay * bz - az * by;
    sy += az * bx - ax * bz;
    sz += ax * by - ay * bx;
  }
  const float len = sqrtf(sx * sx + sy * sy + sz * sz);
  const float inv = len > 0.f ? 1.f / len : 0.f;
  o[0] = sx * inv;
  o[1] = sy * inv;
  o[2] = sz * inv;
}
__global__ __launch_bounds__(256) void render_vnormal_kernel(RndTab tab, const int* __restrict__ faces, const int* __restrict__ adj_ptr,
                                                             const int* __restrict__ adj_idx, int V, int F, float* __restrict__ vnorm) {
  const int v = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
  if (v >= V) return;
  render_vnormal_body(tab.verts[n], faces, adj_ptr, adj_idx, V, F, vnorm + ((size_t)n * V + v) * 3, v);
}

// ---- face set-up ---------------------------------------------------------------------------------------------------------------
// snapped image position of a vertex; false when it leaves the range the int64 edge functions are safe in
__device__ __forceinline__ bool render_snap(const float* p, float hw, float hh, float sx, float sy, float tx, float ty, int& u, int& v) {
  const float fu = rintf(hw * (1.f + sx * (p[0] + tx)) * 256.f);
  const float fv = rintf(hh * (1.f + sy * (p[1] + ty)) * 256.f);
  // false for NaN as well; a corner whose depth is not finite drops its faces too, so that every depth compared below is ordered
  const bool ok = fabsf(fu) <= RND_SNAP_LIMIT && fabsf(fv) <= RND_SNAP_LIMIT && fabsf(p[2]) < __uint_as_float(0x7f800000u);
  u = ok ? (int)fu : 0;
  v = ok ? (int)fv : 0;
  return ok;
}
// The drawn orientation: corners (a, b, c) = (v0, v2, v1), so that a front face has a positive area below.
__device__ __forceinline__ long long render_edge(int ax, int ay, int bx, int by, int px, int py) {
  // widened before the subtraction: two corners at +-2^30 differ by 2^31
  return ((long long)bx - ax) * ((long long)py - ay) - ((long long)by - ay) * ((long long)px - ax);
}
// top-left rule for the edge a -> b of a positively oriented triangle (x right, y down): a pixel centre ON the edge is inside
// when the edge is a left edge (it runs upwards) or a top edge (horizontal, running right)
__device__ __forceinline__ bool render_owns_edge(int ax, int ay, int bx, int by) { return by < ay || (by == ay && bx > ax); }

// face f of the mesh at P under the camera (sx, sy, tx, ty) on an H x W frame -> its snapped corners c[6] and pixel box b[2]
__device__ __forceinline__ void render_face_setup_body(const float* __restrict__ P, const int* __restrict__ faces, float sx, float sy,
                                                       float tx, float ty, int V, int H, int W, int* __restrict__ c,
                                                       int* __restrict__ b, int f) {
  const float hw = 0.5f * (float)W, hh = 0.5f * (float)H;
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  int x0 = 0, y0 = 0, x1 = 0, y1 = 0, x2 = 0, y2 = 0;
  bool ok = (unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V;
  if (ok) {
    ok = render_snap(P + 3 * i0, hw, hh, sx, sy, tx, ty, x0, y0);
    ok = render_snap(P + 3 * i1, hw, hh, sx, sy, tx, ty, x1, y1) && ok;
    ok = render_snap(P + 3 * i2, hw, hh, sx, sy, tx, ty, x2, y2) && ok;
  }
  int bx = RND_EMPTY_BOX, by = RND_EMPTY_BOX;
  if (ok && render_edge(x0, y0, x2, y2, x1, y1) > 0) {
    const int xmin = rnd_min(x0, rnd_min(x1, x2)), xmax = rnd_max(x0, rnd_max(x1, x2));
    const int ymin = rnd_min(y0, rnd_min(y1, y2)), ymax = rnd_max(y0, rnd_max(y1, y2));
    // pixel i has its centre at 256 i + 128: the pixels whose centre lies in [min, max]
    int ilo = (xmin + 127) >> 8, ihi = (xmax - 128) >> 8, jlo = (ymin + 127) >> 8, jhi = (ymax - 128) >> 8;
    ilo = rnd_max(ilo, 0);
    ihi = rnd_min(ihi, W - 1);
    jlo = rnd_max(jlo, 0);
    jhi = rnd_min(jhi, H - 1);
    if (ilo <= ihi && jlo <= jhi) {
      bx = ilo | (ihi << 16);
      by = jlo | (jhi << 16);
    }
  }
  c[0] = x0; c[1] = y0; c[2] = x1; c[3] = y1; c[4] = x2; c[5] = y2;
  b[0] = bx;
  b[1] = by;
}
// a mesh is set up on its scene's frame size
__global__ __launch_bounds__(256) void render_face_setup_kernel(RndTab tab, const int* __restrict__ faces, const float* __restrict__ cam,
                                                                int V, int F, int* __restrict__ fcoord, int* __restrict__ fbox) {
  const int f = blockIdx.x * 256 + threadIdx.x, n = blockIdx.z;
  if (f >= F) return;
  const size_t g = (size_t)n * F + f;
  const int k = tab.scene_of[n];
  render_face_setup_body(tab.verts[n], faces, cam[4 * n], cam[4 * n + 1], cam[4 * n + 2], cam[4 * n + 3], V, tab.s[k].H, tab.s[k].W,
                         fcoord + g * 6, fbox + 2 * g, f);
}

// ---- pixel box of a whole mesh (ragged and scene entries) ------------------------------------------------------------------------
// One workgroup per mesh: the union of its faces' pixel boxes, reduced in LDS with integer min / max - deterministic, no atomics.
// mbox[4 n ..] = xlo, xhi, ylo, yhi; a mesh with no drawn face keeps the empty box (xlo > xhi).
__global__ __launch_bounds__(256) void render_mesh_box_kernel(const int* __restrict__ fbox, int F, int* __restrict__ mbox) {
  __shared__ int s_b[4][256];
  const int t = threadIdx.x, n = blockIdx.x;
  const int* B = fbox + (size_t)n * F * 2;
  int xlo = 65535, xhi = -1, ylo = 65535, yhi = -1;
  for (int f = t; f < F; f += 256) {
    const int bx = B[2 * f], by = B[2 * f + 1];
    if ((bx & 0xffff) > (bx >> 16) || (by & 0xffff) > (by >> 16)) continue;      // culled / off the frame
    xlo = rnd_min(xlo, bx & 0xffff); xhi = rnd_max(xhi, bx >> 16);
    ylo = rnd_min(ylo, by & 0xffff); yhi = rnd_max(yhi, by >> 16);
  }
  s_b[0][t] = xlo; s_b[1][t] = xhi; s_b[2][t] = ylo; s_b[3][t] = yhi;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (t < w) {
      s_b[0][t] = rnd_min(s_b[0][t], s_b[0][t + w]); s_b[1][t] = rnd_max(s_b[1][t], s_b[1][t + w]);
      s_b[2][t] = rnd_min(s_b[2][t], s_b[2][t + w]); s_b[3][t] = rnd_max(s_b[3][t], s_b[3][t + w]);
    }
    __syncthreads();
  }
  if (t < 4) mbox[4 * n + t] = s_b[t][0];
}

// ---- one workgroup per 16x16 tile ----------------------------------------------------------------------------------------------
struct RenderHit {
  long long wa, wb, wc, area;      // weights of v0, v2, v1 (the drawn orientation) and their sum
};
// coverage of the pixel centre (px, py), in snapped units, by the face with corners v0 = (x0, y0), v1, v2
__device__ __forceinline__ bool render_cover(int x0, int y0, int x1, int y1, int x2, int y2, int px, int py, RenderHit& h) {
  // a = v0, b = v2, c = v1
  h.wa = render_edge(x2, y2, x1, y1, px, py);      // edge b -> c, weight of a
  h.wb = render_edge(x1, y1, x0, y0, px, py);      // edge c -> a, weight of b
  h.wc = render_edge(x0, y0, x2, y2, px, py);      // edge a -> b, weight of c
  h.area = h.wa + h.wb + h.wc;
  const long long ea = h.wa - (render_owns_edge(x2, y2, x1, y1) ? 0 : 1);
  const long long eb = h.wb - (render_owns_edge(x1, y1, x0, y0) ? 0 : 1);
  const long long ec = h.wc - (render_owns_edge(x0, y0, x2, y2) ? 0 : 1);
  return (ea | eb | ec) >= 0;
}

// the wire rule for a covered centre: within one pixel of one of the face's edges, along that edge's minor axis
__device__ __forceinline__ long long render_edge_reach(int ax, int ay, int bx, int by) {
  long long dx = (long long)bx - ax, dy = (long long)by - ay;
  dx = dx < 0 ? -dx : dx;
  dy = dy < 0 ? -dy : dy;
  return 256 * (dx > dy ? dx : dy);
}
__device__ __forceinline__ bool render_on_wire(int x0, int y0, int x1, int y1, int x2, int y2, const RenderHit& h) {
  return h.wa < render_edge_reach(x2, y2, x1, y1) || h.wb < render_edge_reach(x1, y1, x0, y0) ||
         h.wc < render_edge_reach(x0, y0, x2, y2);
}

// The frame under a tile -> the tile's LDS picture s_px, and back: 16-byte rows when the layout allows it (`wide`: W a multiple of 16
// and 16-byte aligned bases), else one pixel per thread.  bg NULL: black.  The callers put a barrier between either of them and
// any other use of s_px.
__device__ __forceinline__ void render_frame_load(uint8_t (*s_px)[RND_TILE * 3], const uint8_t* __restrict__ bg, int H, int W, int wide,
                                                  int tx0, int ty0, int t, int lx, int ly, int i, int j, bool live) {
  if (wide) {
    if (t < 3 * RND_TILE) {
      const int r = t / 3, q = t - 3 * r;
      rnd_u32x4 v = {0u, 0u, 0u, 0u};
      if (bg && ty0 + r < H) v = *reinterpret_cast<const rnd_u32x4*>(bg + ((size_t)(ty0 + r) * W + tx0) * 3 + 16 * q);
      *reinterpret_cast<rnd_u32x4*>(&s_px[r][16 * q]) = v;
    }
  } else {
    const uint8_t* s = bg && live ? bg + ((size_t)j * W + i) * 3 : nullptr;
    s_px[ly][3 * lx] = s ? s[0] : 0;
    s_px[ly][3 * lx + 1] = s ? s[1] : 0;
    s_px[ly][3 * lx + 2] = s ? s[2] : 0;
  }
}
__device__ __forceinline__ void render_frame_store(uint8_t (*s_px)[RND_TILE * 3], uint8_t* __restrict__ out, int H, int W, int wide,
                                                   int tx0, int ty0, int t, int lx, int ly, int i, int j, bool live) {
  if (wide) {
    if (t < 3 * RND_TILE) {
      const int r = t / 3, q = t - 3 * r;
      if (ty0 + r < H)
        *reinterpret_cast<rnd_u32x4*>(out + ((size_t)(ty0 + r) * W + tx0) * 3 + 16 * q) =
            *reinterpret_cast<const rnd_u32x4*>(&s_px[r][16 * q]);
    }
  } else if (live) {
    uint8_t* o = out + ((size_t)j * W + i) * 3;
    o[0] = s_px[ly][3 * lx];
    o[1] = s_px[ly][3 * lx + 1];
    o[2] = s_px[ly][3 * lx + 2];
  }
}
// The colour of the pixel centre (px, py) where face f of the mesh (P, N its vertex rows and normals, C its snapped corners) won:
// smooth shading as the header states it -> rgb[3].  The one statement of that arithmetic: every tile kernel shades through it.
__device__ __forceinline__ void render_shade(const float* __restrict__ P, const int* __restrict__ faces, const float* __restrict__ N,
                                             const int* __restrict__ C, int f, int px, int py, float cr, float cg, float cb,
                                             uint8_t* rgb) {
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  const int* c = C + 6 * (size_t)f;
  RenderHit h;
  render_cover(c[0], c[1], c[2], c[3], c[4], c[5], px, py, h);
  const float ar = (float)h.area;
  const float b0 = (float)h.wa / ar, b1 = (float)h.wc / ar, b2 = (float)h.wb / ar;
  float nx = b0 * N[3 * i0] + b1 * N[3 * i1] + b2 * N[3 * i2];
  float ny = b0 * N[3 * i0 + 1] + b1 * N[3 * i1 + 1] + b2 * N[3 * i2 + 1];
  float nz = b0 * N[3 * i0 + 2] + b1 * N[3 * i1 + 2] + b2 * N[3 * i2 + 2];
  const float nl = sqrtf(nx * nx + ny * ny + nz * nz);
  const float ni = nl > 0.f ? 1.f / nl : 0.f;
  // the turned space: (x, -y, -z) for positions and normals alike
  nx = nx * ni;
  ny = -(ny * ni);
  nz = -(nz * ni);
  const float qx = b0 * P[3 * i0] + b1 * P[3 * i1] + b2 * P[3 * i2];
  const float qy = -(b0 * P[3 * i0 + 1] + b1 * P[3 * i1 + 1] + b2 * P[3 * i2 + 1]);
  const float qz = -(b0 * P[3 * i0 + 2] + b1 * P[3 * i1 + 2] + b2 * P[3 * i2 + 2]);
  const float L[3][3] = {{0.f, -1.f, 1.f}, {0.f, 1.f, 1.f}, {1.f, 1.f, 2.f}};
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float dx = L[k][0] - qx, dy = L[k][1] - qy, dz = L[k][2] - qz;
    const float dl = sqrtf(dx * dx + dy * dy + dz * dz);
    const float dot = dl > 0.f ? (nx * dx + ny * dy + nz * dz) / dl : 0.f;
    sum += fmaxf(dot, 0.f);
  }
  const float I = fminf(0.3f + 0.35f * sum, 1.f);
  rgb[0] = (uint8_t)fminf(fmaxf(rintf(255.f * I * cr), 0.f), 255.f);
  rgb[1] = (uint8_t)fminf(fmaxf(rintf(255.f * I * cg), 0.f), 255.f);
  rgb[2] = (uint8_t)fminf(fmaxf(rintf(255.f * I * cb), 0.f), 255.f);
}

// One chunk of a mesh's face list over the tile (tx0 .. tx1, ty0 .. ty1): faces c * 256 .. of the mesh (P, C, B as in the tile body)
// whose box touches the tile are compacted into LDS with their corners and depths, and a pixel that takes part (`test`) keeps the
// nearest face covering it in (best, best_f); ties go to the lower face index.  g: the running number of the chunk in this workgroup
// - the LDS entries are double-buffered and the counters rotate by it (g = c for one mesh; a workgroup that walks several meshes
// goes on counting).  Every thread of the workgroup calls it: it holds a barrier.  WIRE: only the fragments of the wire rule count.
template <bool WIRE>
__device__ __forceinline__ void render_chunk_nearest(const float* __restrict__ P, const int* __restrict__ faces, const int* __restrict__ C,
                                                     const int* __restrict__ B, int F, int c, int g, int tx0, int tx1, int ty0, int ty1,
                                                     int t, int i, int j, int px, int py, bool test, int (*s_xy)[6][RND_CHUNK],
                                                     int (*s_box)[2][RND_CHUNK], float (*s_z)[3][RND_CHUNK], int (*s_f)[RND_CHUNK],
                                                     unsigned* s_cnt, float& best, int& best_f) {
  const int buf = g & 1, cn = g % 3;
  // counter of the next chunk: last read two chunks ago, before the barrier every thread has passed since
  if (t == 0) s_cnt[(g + 1) % 3] = 0;
  const int f = c * RND_CHUNK + t;
  if (f < F) {
    const int bx = B[2 * f], by = B[2 * f + 1];
    if ((bx & 0xffff) <= tx1 && (bx >> 16) >= tx0 && (by & 0xffff) <= ty1 && (by >> 16) >= ty0) {
      const unsigned s = atomicAdd(&s_cnt[cn], 1u);
      const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];      // in range: set-up gave a box
#pragma unroll
      for (int k = 0; k < 6; ++k) s_xy[buf][k][s] = C[6 * (size_t)f + k];
      s_box[buf][0][s] = bx;
      s_box[buf][1][s] = by;
      s_z[buf][0][s] = P[3 * i0 + 2];
      s_z[buf][1][s] = P[3 * i1 + 2];
      s_z[buf][2][s] = P[3 * i2 + 2];
      s_f[buf][s] = f;
    }
  }
  __syncthreads();
  const int m = (int)s_cnt[cn];
  if (test) {
    for (int e = 0; e < m; ++e) {
      const int bx = s_box[buf][0][e], by = s_box[buf][1][e];
      if (i < (bx & 0xffff) || i > (bx >> 16) || j < (by & 0xffff) || j > (by >> 16)) continue;
      RenderHit h;
      if (!render_cover(s_xy[buf][0][e], s_xy[buf][1][e], s_xy[buf][2][e], s_xy[buf][3][e], s_xy[buf][4][e], s_xy[buf][5][e], px,
                        py, h))
        continue;
      if (WIRE && !render_on_wire(s_xy[buf][0][e], s_xy[buf][1][e], s_xy[buf][2][e], s_xy[buf][3][e], s_xy[buf][4][e],
                                  s_xy[buf][5][e], h))
        continue;
      // weights of v0, v1, v2 = wa, wc, wb
      const float d = ((float)h.wa * s_z[buf][0][e] + (float)h.wc * s_z[buf][1][e] + (float)h.wb * s_z[buf][2][e]) / (float)h.area;
      const int f2 = s_f[buf][e];
      if (d < best || (d == best && f2 < best_f) || best_f < 0) {
        best = d;
        best_f = f2;
      }
    }
  }
  // the entries of this chunk are overwritten two chunks on, behind the next barrier
}

// One workgroup per tile of a scene, on a flat grid over the prefix of the scenes' tile counts: workgroup -> (scene, tile) by a search
// of the prefix.  Each mesh of a scene has its own weak-perspective camera: the Z of two people is measured about two pelvises and
// cannot be compared, so there is NO depth test between meshes.  Within a mesh the nearest face wins (ties: the lower index), between
// meshes the one listed later wins wherever it covers the pixel - what the chain  img = render(img, mesh_i)  over the list draws,
// byte for byte.  The workgroup walks the scene's meshes from the last (on top) to the first: a mesh whose pixel box misses the tile
// (use_box) is passed over, a pixel is decided by the first mesh it meets that covers it, a decided pixel makes no more coverage
// tests, and the walk ends when every live pixel of the tile is decided.  The pixel is shaded once, at the end, with the winner's
// vertex rows, normals and colour: colors[3 m ..], or (cr, cg, cb) for every mesh when colors is NULL (the uniform and ragged
// entries pass one colour as scalars and allocate nothing).  depth (uniform entry only: its scenes share one H x W, scene k's map
// lies at depth + k H W): the winning face's depth, +inf where nothing is drawn.  WIRE: the wireframe variant of the same body - a mesh
// claims the pixels where it has a wire fragment only, so a tile a mesh covers without wires goes on to the mesh beneath.
template <bool WIRE>
__global__ __launch_bounds__(256) void render_tile_kernel(RndTab tab, int nscenes, const int* __restrict__ faces,
                                                          const float* __restrict__ vnorm, const int* __restrict__ fcoord,
                                                          const int* __restrict__ fbox, const int* __restrict__ mbox,
                                                          const float* __restrict__ colors, float* __restrict__ depth, float cr,
                                                          float cg, float cb, int V, int F, int use_box) {
  __shared__ int s_xy[2][6][RND_CHUNK];
  __shared__ int s_box[2][2][RND_CHUNK];
  __shared__ float s_z[2][3][RND_CHUNK];
  __shared__ int s_f[2][RND_CHUNK];
  __shared__ unsigned s_cnt[3];
  __shared__ unsigned s_decided;
  __shared__ __attribute__((aligned(16))) uint8_t s_px[RND_TILE][RND_TILE * 3];
  const int bid = (int)blockIdx.x;
  int lo = 0, hi = nscenes;                     // the scene k with tile0[k] <= bid < tile0[k + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tab.tile0[mid] <= bid) lo = mid;
    else hi = mid;
  }
  const RndScene sc = tab.s[lo];
  const int H = sc.H, W = sc.W;
  const int tw = (W + RND_TILE - 1) / RND_TILE, local = bid - tab.tile0[lo];
  const int tyi = local / tw, txi = local - tyi * tw;
  const int tx0 = txi * RND_TILE, ty0 = tyi * RND_TILE;
  // decided per scene; for the uniform entry one decision for the call, as its images lie n H W 3 bytes apart: a multiple of 16
  // whenever W is
  const int wide = W % 16 == 0 && ((uintptr_t)sc.out & 15) == 0 && ((uintptr_t)sc.bg & 15) == 0;
  const int t = threadIdx.x;
  const int tx1 = rnd_min(tx0 + RND_TILE, W) - 1, ty1 = rnd_min(ty0 + RND_TILE, H) - 1;
  const int lx = t & (RND_TILE - 1), ly = t >> 4;
  const int i = tx0 + lx, j = ty0 + ly;
  const bool live = i < W && j < H;
  const int px = 256 * i + 128, py = 256 * j + 128;
  const unsigned nlive = (unsigned)((tx1 - tx0 + 1) * (ty1 - ty0 + 1));
  render_frame_load(s_px, sc.bg, H, W, wide, tx0, ty0, t, lx, ly, i, j, live);
  if (t < 3) s_cnt[t] = 0;
  if (t == 0) s_decided = 0;
  __syncthreads();

  int win_m = -1, win_f = -1;                   // the mesh (index in the call's list) and the face this pixel shows
  float win_d = __uint_as_float(0x7f800000u);   // ... and its depth there; +inf: nothing
  const int nchunks = (F + RND_CHUNK - 1) / RND_CHUNK;
  int g = 0;                                    // chunks streamed so far, over all meshes
  for (int m = (int)sc.m1 - 1; m >= (int)sc.m0; --m) {
    if (use_box) {                              // the same for the whole workgroup
      const int xlo = mbox[4 * m], xhi = mbox[4 * m + 1], ylo = mbox[4 * m + 2], yhi = mbox[4 * m + 3];
      if (xlo > xhi || xlo > tx1 || xhi < tx0 || ylo > ty1 || yhi < ty0) continue;
    }
    const float* P = tab.verts[m];
    const int* C = fcoord + (size_t)m * F * 6;
    const int* B = fbox + (size_t)m * F * 2;
    float best = __uint_as_float(0x7f800000u);
    int best_f = -1;
    // a decided pixel tests nothing, but goes through the barriers with the others
    for (int c = 0; c < nchunks; ++c, ++g)
      render_chunk_nearest<WIRE>(P, faces, C, B, F, c, g, tx0, tx1, ty0, ty1, t, i, j, px, py, live && win_m < 0, s_xy, s_box, s_z, s_f, s_cnt,
                                 best, best_f);
    const bool won = live && win_m < 0 && best_f >= 0;
    if (won) {
      win_m = m;
      win_f = best_f;
      win_d = best;
    }
    // the bottom mesh of the scene (the only one of a uniform or ragged picture): no walk is left to end, nobody needs the count
    if (m == (int)sc.m0) break;
    if (won) atomicAdd(&s_decided, 1u);
    // read behind the barrier: one value for the whole workgroup.  The next addition to it lies behind a barrier of the next mesh's
    // first chunk, which no thread passes before all have read it here.
    __syncthreads();
    if (s_decided == nlive) break;
  }

  if (live && win_m >= 0)
    render_shade(tab.verts[win_m], faces, vnorm + (size_t)win_m * V * 3, fcoord + (size_t)win_m * F * 6, win_f, px, py,
                 colors ? colors[3 * win_m] : cr, colors ? colors[3 * win_m + 1] : cg, colors ? colors[3 * win_m + 2] : cb,
                 &s_px[ly][3 * lx]);
  if (live) {
    if (sc.mesh_id) sc.mesh_id[(size_t)j * W + i] = win_m >= 0 ? win_m - (int)sc.m0 : -1;
    if (sc.face_id) sc.face_id[(size_t)j * W + i] = win_f;
    if (depth) depth[((size_t)lo * H + j) * W + i] = win_d;
  }
  __syncthreads();
  render_frame_store(s_px, sc.out, H, W, wide, tx0, ty0, t, lx, ly, i, j, live);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// scratch: vertex normals [N][V][3] fp32 (first, so a caller can read them back), snapped corners [N][F][6] int32, boxes [N][F][2] int32
extern "C" size_t dyb_render_workspace_bytes(int N, int V, int F) {
  if (N <= 0 || V <= 0 || F <= 0) return 0;
  return rnd_align((size_t)N * V * 3 * sizeof(float)) + rnd_align((size_t)N * F * 6 * sizeof(int)) +
         rnd_align((size_t)N * F * 2 * sizeof(int));
}
// scratch of the ragged entry: as above, then the meshes' pixel boxes [N][4] int32
extern "C" size_t dyb_render_var_workspace_bytes(int N, int V, int F) {
  if (N <= 0 || V <= 0 || F <= 0) return 0;
  return dyb_render_workspace_bytes(N, V, F) + rnd_align((size_t)N * 4 * sizeof(int));
}
// scratch of the scene entry: that of the ragged entry for nmeshes meshes; none without a mesh
extern "C" size_t dyb_render_scenes_workspace_bytes(int nmeshes, int V, int F) { return dyb_render_var_workspace_bytes(nmeshes, V, F); }
// what a call with opts->model needs on top of its entry's own scratch, behind it: the turned vertices [N][V][3] fp32
extern "C" size_t dyb_render_model_workspace_bytes(int N, int V) {
  if (N <= 0 || V <= 0) return 0;
  return rnd_align((size_t)N * V * 3 * sizeof(float));
}

// The matrices of a call, checked on the host before anything is launched: M x 9 floats come over on the call's stream, which is
// waited for (calls without matrices never wait).  DYB_ERR_ARG for an entry that is not finite.
static int render_check_model(const float* model, int M, hipStream_t st) {
  float h[RND_MAX_N * 9];
  if (hipMemcpyAsync(h, model, (size_t)M * 9 * sizeof(float), hipMemcpyDeviceToHost, st) != hipSuccess) return DYB_ERR_LAUNCH;
  if (hipStreamSynchronize(st) != hipSuccess) return DYB_ERR_LAUNCH;
  for (int k = 0; k < 9 * M; ++k) DYB_REQUIRE(fabsf(h[k]) < __builtin_inff(), DYB_ERR_ARG);      // false for NaN as well
  return DYB_OK;
}

// The launches of a checked call: the table's tile prefix is filled in, the workspace carved (the one statement of its layout: the
// workspace_bytes functions above count these parts) and the kernels issued - with matrices the pre-pass, after which the table
// names the turned rows; normals, face set-up and, with use_box, the mesh boxes for the M meshes of the list, then the tiles of the
// nscenes scenes.  use_box = 0: the workspace need not hold the mesh boxes.  base: the bytes of the entry's own scratch - the turned
// rows lie behind them.
static int render_launch(RndTab& tab, int nscenes, int M, const int* faces, const int* adj_ptr, const int* adj_idx, const float* cam,
                         const float* colors, float cr, float cg, float cb, float* depth, int V, int F, int use_box, void* ws,
                         size_t base, const dyb_render_opts* opts, hipStream_t st) {
  long long tiles = 0;
  for (int k = 0; k <= RND_MAX_N; ++k) {
    tab.tile0[k] = (int)tiles;
    if (k < nscenes) tiles += (long long)dyb_cdiv(tab.s[k].W, RND_TILE) * dyb_cdiv(tab.s[k].H, RND_TILE);      // <= 64 * 256 * 256: inside int and a 1-D grid
  }
  char* w = reinterpret_cast<char*>(ws);
  float* vnorm = reinterpret_cast<float*>(w);
  w += rnd_align((size_t)M * V * 3 * sizeof(float));
  int* fcoord = reinterpret_cast<int*>(w);
  w += rnd_align((size_t)M * F * 6 * sizeof(int));
  int* fbox = reinterpret_cast<int*>(w);
  w += rnd_align((size_t)M * F * 2 * sizeof(int));
  int* mbox = use_box ? reinterpret_cast<int*>(w) : nullptr;
  if (M > 0) {
    if (opts && opts->model) {
      float* turned = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + base);
      hipLaunchKernelGGL(render_transform_tab_kernel, dim3(dyb_cdiv(V, 256), 1, M), dim3(256), 0, st, tab, opts->model, V, turned);
      DYB_CHECK_LAUNCH();
      for (int m = 0; m < M; ++m) tab.verts[m] = turned + (size_t)m * V * 3;
    }
    hipLaunchKernelGGL(render_vnormal_kernel, dim3(dyb_cdiv(V, 256), 1, M), dim3(256), 0, st, tab, faces, adj_ptr, adj_idx, V, F, vnorm);
    DYB_CHECK_LAUNCH();
    hipLaunchKernelGGL(render_face_setup_kernel, dim3(dyb_cdiv(F, 256), 1, M), dim3(256), 0, st, tab, faces, cam, V, F, fcoord, fbox);
    DYB_CHECK_LAUNCH();
    if (use_box) {
      hipLaunchKernelGGL(render_mesh_box_kernel, dim3(M), dim3(256), 0, st, (const int*)fbox, F, mbox);
      DYB_CHECK_LAUNCH();
    }
  }
  if (opts && opts->wireframe)
    hipLaunchKernelGGL(render_tile_kernel<true>, dim3((unsigned)tiles), dim3(256), 0, st, tab, nscenes, faces, (const float*)vnorm,
                       (const int*)fcoord, (const int*)fbox, (const int*)mbox, colors, depth, cr, cg, cb, V, F, use_box);
  else
    hipLaunchKernelGGL(render_tile_kernel<false>, dim3((unsigned)tiles), dim3(256), 0, st, tab, nscenes, faces, (const float*)vnorm,
                       (const int*)fcoord, (const int*)fbox, (const int*)mbox, colors, depth, cr, cg, cb, V, F, use_box);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}
// the last checks of an entry (they wait for the stream when there are matrices, so they come after every other check), then the launches
static int render_checked_launch(RndTab& tab, int nscenes, int M, const int* faces, const int* adj_ptr, const int* adj_idx,
                                 const float* cam, const float* colors, float cr, float cg, float cb, float* depth, int V, int F,
                                 int use_box, void* ws, size_t ws_bytes, size_t base, const dyb_render_opts* opts, hipStream_t st) {
  const bool turned = opts && opts->model && M > 0;
  DYB_REQUIRE(ws_bytes >= base + (turned ? dyb_render_model_workspace_bytes(M, V) : 0), DYB_ERR_WORKSPACE);
  if (turned) {
    const int rc = render_check_model(opts->model, M, st);
    if (rc != DYB_OK) return rc;
  }
  return render_launch(tab, nscenes, M, faces, adj_ptr, adj_idx, cam, colors, cr, cg, cb, depth, V, F, use_box, ws, base, opts, st);
}

// ---- the matrix arithmetic on its own ----------------------------------------------------------------------------------------------
// out [N][V][3] = model[n] verts[n][v], the arithmetic the entries apply with opts->model; model NULL: out = verts, bit for bit.
extern "C" int dyb_render_transform_verts(const float* verts, const float* model, float* out, int N, int V, hipStream_t st) {
  DYB_REQUIRE(verts && out, DYB_ERR_ARG);
  DYB_REQUIRE(N > 0 && V > 0, DYB_ERR_ARG);
  DYB_REQUIRE(V <= (1 << 28) && (long long)N * V <= (1LL << 31), DYB_ERR_UNSUPPORTED);       // the flat grid stays inside 2^23 workgroups
  const long long total = (long long)N * V;
  hipLaunchKernelGGL(render_transform_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, verts, model, out, total, V);
  DYB_CHECK_LAUNCH();
  return DYB_OK;
}

// ---- the uniform entry: N meshes, one frame size, strided images -----------------------------------------------------------------
// No pixel box: three launches, and the workspace has no room for the mesh boxes.
extern "C" int dyb_render_meshes_opt(const float* verts, const int* faces, const int* adj_ptr, const int* adj_idx, const float* cam,
                                     const uint8_t* background, float col_r, float col_g, float col_b, uint8_t* out, int* face_id,
                                     float* depth, int N, int V, int F, int H, int W, void* ws, size_t ws_bytes, hipStream_t st,
                                     const dyb_render_opts* opts) {
  DYB_REQUIRE(verts && faces && adj_ptr && adj_idx && cam && out && ws, DYB_ERR_ARG);
  DYB_REQUIRE(N > 0 && V > 0 && F > 0 && H > 0 && W > 0, DYB_ERR_ARG);
  DYB_REQUIRE(N <= RND_MAX_N && H <= RND_MAX_DIM && W <= RND_MAX_DIM, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(F <= (1 << 28) && V <= (1 << 28), DYB_ERR_UNSUPPORTED);                  // 3 F and 3 V stay inside int
  RndTab tab{};
  const size_t img = (size_t)H * W;
  for (int n = 0; n < N; ++n) {
    tab.s[n] = RndScene{background ? background + n * img * 3 : nullptr, out + n * img * 3, nullptr, face_id ? face_id + n * img : nullptr,
                        (unsigned short)H, (unsigned short)W, (unsigned char)n, (unsigned char)(n + 1)};
    tab.verts[n] = verts + (size_t)n * V * 3;
    tab.scene_of[n] = (unsigned char)n;
  }
  return render_checked_launch(tab, N, N, faces, adj_ptr, adj_idx, cam, nullptr, col_r, col_g, col_b, depth, V, F, 0, ws, ws_bytes,
                               dyb_render_workspace_bytes(N, V, F), opts, st);
}
extern "C" int dyb_render_meshes(const float* verts, const int* faces, const int* adj_ptr, const int* adj_idx, const float* cam,
                                 const uint8_t* background, float col_r, float col_g, float col_b, uint8_t* out, int* face_id,
                                 float* depth, int N, int V, int F, int H, int W, void* ws, size_t ws_bytes, hipStream_t st) {
  return dyb_render_meshes_opt(verts, faces, adj_ptr, adj_idx, cam, background, col_r, col_g, col_b, out, face_id, depth, N, V, F, H, W, ws,
                               ws_bytes, st, nullptr);
}

// ---- the ragged entry: every mesh with its own frame size and pointers ----------------------------------------------------------
// desc: HOST table of N entries (copied into the launches' kernel arguments: free to reuse when the call returns).  flags bit 0:
// leave the per-mesh pixel box out (every tile streams the face list, as the uniform entry does; same bytes - for measurements).
extern "C" int dyb_render_meshes_var_opt(const dyb_render_desc* desc, const int* faces, const int* adj_ptr, const int* adj_idx,
                                         const float* cam, float col_r, float col_g, float col_b, int N, int V, int F, int flags,
                                         void* ws, size_t ws_bytes, hipStream_t st, const dyb_render_opts* opts) {
  DYB_REQUIRE(desc && faces && adj_ptr && adj_idx && cam && ws, DYB_ERR_ARG);
  DYB_REQUIRE(N > 0 && V > 0 && F > 0, DYB_ERR_ARG);
  DYB_REQUIRE(N <= RND_MAX_N, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(F <= (1 << 28) && V <= (1 << 28), DYB_ERR_UNSUPPORTED);
  RndTab tab{};
  for (int n = 0; n < N; ++n) {
    const dyb_render_desc& d = desc[n];
    DYB_REQUIRE(d.verts && d.out && d.H > 0 && d.W > 0, DYB_ERR_ARG);
    DYB_REQUIRE(d.H <= RND_MAX_DIM && d.W <= RND_MAX_DIM, DYB_ERR_UNSUPPORTED);
    tab.s[n] = RndScene{d.background, d.out, nullptr, nullptr, (unsigned short)d.H, (unsigned short)d.W, (unsigned char)n,
                        (unsigned char)(n + 1)};
    tab.verts[n] = d.verts;
    tab.scene_of[n] = (unsigned char)n;
  }
  return render_checked_launch(tab, N, N, faces, adj_ptr, adj_idx, cam, nullptr, col_r, col_g, col_b, nullptr, V, F, (flags & 1) ? 0 : 1, ws,
                               ws_bytes, dyb_render_var_workspace_bytes(N, V, F), opts, st);
}
extern "C" int dyb_render_meshes_var(const dyb_render_desc* desc, const int* faces, const int* adj_ptr, const int* adj_idx,
                                     const float* cam, float col_r, float col_g, float col_b, int N, int V, int F, int flags, void* ws,
                                     size_t ws_bytes, hipStream_t st) {
  return dyb_render_meshes_var_opt(desc, faces, adj_ptr, adj_idx, cam, col_r, col_g, col_b, N, V, F, flags, ws, ws_bytes, st, nullptr);
}

// ---- the scene entry: several meshes over ONE frame, in painter order ------------------------------------------------------------
// scenes: HOST table of nscenes entries; mesh_verts: HOST table of nmeshes device pointers; mesh_scene: HOST table, the scene of
// each mesh (it must agree with the scenes' ranges, which must tile 0 .. nmeshes in order).  Both are copied into the launches'
// kernel arguments.  flags bit 0: leave the per-mesh pixel boxes out (same bytes - for measurements).  Without a mesh (ws may be
// NULL) only the tiles are launched: they copy the frames.
extern "C" int dyb_render_scenes_opt(const dyb_render_scene* scenes, int nscenes, const float* const* mesh_verts, const int* mesh_scene,
                                     const float* cam, const float* colors, const int* faces, const int* adj_ptr, const int* adj_idx,
                                     int nmeshes, int V, int F, int flags, void* ws, size_t ws_bytes, hipStream_t st,
                                     const dyb_render_opts* opts) {
  DYB_REQUIRE(scenes && faces && adj_ptr && adj_idx, DYB_ERR_ARG);
  DYB_REQUIRE(nscenes > 0 && nmeshes >= 0 && V > 0 && F > 0, DYB_ERR_ARG);
  DYB_REQUIRE(nmeshes == 0 || (mesh_verts && mesh_scene && cam && colors && ws), DYB_ERR_ARG);
  DYB_REQUIRE(nscenes <= RND_MAX_N && nmeshes <= RND_MAX_N, DYB_ERR_UNSUPPORTED);
  DYB_REQUIRE(F <= (1 << 28) && V <= (1 << 28), DYB_ERR_UNSUPPORTED);
  RndTab tab{};
  int next = 0;
  for (int k = 0; k < nscenes; ++k) {
    const dyb_render_scene& d = scenes[k];
    DYB_REQUIRE(d.out && d.H > 0 && d.W > 0, DYB_ERR_ARG);
    DYB_REQUIRE(d.mesh_begin == next && d.mesh_end >= d.mesh_begin && d.mesh_end <= nmeshes, DYB_ERR_ARG);
    DYB_REQUIRE(d.H <= RND_MAX_DIM && d.W <= RND_MAX_DIM, DYB_ERR_UNSUPPORTED);
    next = d.mesh_end;
    tab.s[k] = RndScene{d.background, d.out, d.mesh_id, d.face_id, (unsigned short)d.H, (unsigned short)d.W,
                        (unsigned char)d.mesh_begin, (unsigned char)d.mesh_end};
    for (int m = d.mesh_begin; m < d.mesh_end; ++m) {
      DYB_REQUIRE(mesh_verts[m] && mesh_scene[m] == k, DYB_ERR_ARG);
      tab.verts[m] = mesh_verts[m];
      tab.scene_of[m] = (unsigned char)k;
    }
  }
  DYB_REQUIRE(next == nmeshes, DYB_ERR_ARG);
  // with no mesh the colours may be NULL; the tile kernel then never reads a colour
  return render_checked_launch(tab, nscenes, nmeshes, faces, adj_ptr, adj_idx, cam, colors, 0.f, 0.f, 0.f, nullptr, V, F,
                               (flags & 1) ? 0 : 1, ws, ws_bytes, dyb_render_scenes_workspace_bytes(nmeshes, V, F), opts, st);
}
extern "C" int dyb_render_scenes(const dyb_render_scene* scenes, int nscenes, const float* const* mesh_verts, const int* mesh_scene,
                                 const float* cam, const float* colors, const int* faces, const int* adj_ptr, const int* adj_idx,
                                 int nmeshes, int V, int F, int flags, void* ws, size_t ws_bytes, hipStream_t st) {
  return dyb_render_scenes_opt(scenes, nscenes, mesh_verts, mesh_scene, cam, colors, faces, adj_ptr, adj_idx, nmeshes, V, F, flags, ws,
                               ws_bytes, st, nullptr);
}
