// Baseline JPEG on the device (dynaboa_amd/jpeg.py): the rasteriser's [H][W][3] uint8 pictures -> the entropy-coded scan, libjpeg's
// integer arithmetic throughout (include/dynaboa_hip.h states the rules, tests/jpeg_cases.py restates them in NumPy and is itself
// pinned to the scan inside the file PIL writes).  Fixed Annex K tables, so one pass over the picture.  No atomics: every stream word
// and every output byte has one owner, so two calls return equal bytes; grid.y is the picture, so a picture's bytes do not depend on
// its place or company in the batch and the launch count (six) does not grow with N.  A workgroup that has nothing to do in its
// picture (the grid's x extent is the largest picture's) leaves before its first barrier.
//
//   1 jpeg_transform_kernel  one thread per 8x8 block in coding order: colour, 4:2:0 downsample, DCT, quantisation -> 64 int16
//                            coefficients in zig-zag order, the block's quantised DC, the bits of its AC codes
//   2 jpeg_bits_kernel       per tile of 1024 blocks: adds the DC code (difference to the component's previous block) and scans the
//                            bit lengths inside the tile
//   3 jpeg_scan_kernel       one workgroup per picture: exclusive 64-bit prefix of the tile sums, the picture's bit count
//   4 jpeg_emit_kernel       one thread per 32-bit stream word: finds the block that holds the word's first bit in the offset table
//                            (tiles, then blocks), codes blocks from there until the word is full and ORs in the pieces that fall
//                            into it - the owner computes, nothing is shared; counts the word's 0xFF bytes, per tile of 256 words
//   5 jpeg_scan_kernel       prefix of the tiles' 0xFF counts; lengths[i] = bytes + stuffed zeros
//   6 jpeg_stuff_kernel      per tile of 256 words: scans the words' 0xFF counts and writes the bytes, a 0x00 behind every 0xFF,
//                            nothing at or beyond the picture's capacity
//
// The bit count of a picture is known on the device only, so kernel 4 is launched over the worst case (JP_BLOCK_WORDS words per
// block) and sizes the tile arrays; the raw stream in the workspace and kernel 6's grid are bounded by the picture's capacity
// instead: a word beyond it is counted, not stored.
// One thread per block keeps the arithmetic in registers and exact; its byte loads at the row stride and 64 integer divisions are
// not bandwidth-shaped (DESIGN.md section 5 has the measured distance from the memory floor).
#include <stddef.h>

#include <algorithm>

#include "dyb_common.h"

struct dyb_jpeg_desc {                              // include/dynaboa_hip.h; the layout a C caller and the ctypes binding fill
  const uint8_t* rgb;
  uint8_t* out;
  int H, W;
  long long capacity;
};
static_assert(sizeof(dyb_jpeg_desc) == 32 && offsetof(dyb_jpeg_desc, rgb) == 0 && offsetof(dyb_jpeg_desc, out) == 8 &&
                  offsetof(dyb_jpeg_desc, H) == 16 && offsetof(dyb_jpeg_desc, W) == 20 && offsetof(dyb_jpeg_desc, capacity) == 24,
              "dyb_jpeg_desc must keep the layout include/dynaboa_hip.h declares");

#define JP_MAX_N 64
#define JP_MAX_DIM 8192
#define JP_TILE_BLOCKS 1024         // blocks per workgroup of the bits kernel (256 threads x 4)
#define JP_TILE_WORDS 256           // stream words per workgroup of the emit and stuff kernels: 1024 bytes
// A block codes at most 11 + 11 bits of DC and 63 x (16 + 10) bits of AC = 1660 bits; 52 words hold 1664.  (The 7 padding bits of a
// picture fit in the slack: a picture has at least 3 blocks.)
#define JP_BLOCK_WORDS 52
#define JP_DUMMY_DC (-32768)        // in the DC array: a dummy block (4:2:0), whose DC is that of the block before it

// (run << 4 | size) -> length << 16 | code, ITU T.81 Annex K.3.2 tables K.5 (luminance) and K.6 (chrominance)
__device__ const unsigned JP_AC[2][256] = {
  {
    0x4000a, 0x20000, 0x20001, 0x30004, 0x4000b, 0x5001a, 0x70078, 0x800f8, 0xa03f6, 0x10ff82, 0x10ff83, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x4000c, 0x5001b, 0x70079, 0x901f6, 0xb07f6, 0x10ff84, 0x10ff85, 0x10ff86, 0x10ff87, 0x10ff88, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x5001c, 0x800f9, 0xa03f7, 0xc0ff4, 0x10ff89, 0x10ff8a, 0x10ff8b, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003a, 0x901f7, 0xc0ff5, 0x10ff8f, 0x10ff90, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003b, 0xa03f8, 0x10ff96, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x7007a, 0xb07f7, 0x10ff9e, 0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x7007b, 0xc0ff6, 0x10ffa6, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x800fa, 0xc0ff7, 0x10ffae, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f8, 0xf7fc0, 0x10ffb6, 0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f9, 0x10ffbe, 0x10ffbf, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901fa, 0x10ffc7, 0x10ffc8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xa03f9, 0x10ffd0, 0x10ffd1, 0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xa03fa, 0x10ffd9, 0x10ffda, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xb07f8, 0x10ffe2, 0x10ffe3, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x10ffeb, 0x10ffec, 0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0xb07f9, 0x10fff5, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
  },
  {
    0x20000, 0x20001, 0x30004, 0x4000a, 0x50018, 0x50019, 0x60038, 0x70078, 0x901f4, 0xa03f6, 0xc0ff4, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x4000b, 0x60039, 0x800f6, 0x901f5, 0xb07f6, 0xc0ff5, 0x10ff88, 0x10ff89, 0x10ff8a, 0x10ff8b, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x5001a, 0x800f7, 0xa03f7, 0xc0ff6, 0xf7fc2, 0x10ff8c, 0x10ff8d, 0x10ff8e, 0x10ff8f, 0x10ff90, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x5001b, 0x800f8, 0xa03f8, 0xc0ff7, 0x10ff91, 0x10ff92, 0x10ff93, 0x10ff94, 0x10ff95, 0x10ff96, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003a, 0x901f6, 0x10ff97, 0x10ff98, 0x10ff99, 0x10ff9a, 0x10ff9b, 0x10ff9c, 0x10ff9d, 0x10ff9e, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x6003b, 0xa03f9, 0x10ff9f, 0x10ffa0, 0x10ffa1, 0x10ffa2, 0x10ffa3, 0x10ffa4, 0x10ffa5, 0x10ffa6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x70079, 0xb07f7, 0x10ffa7, 0x10ffa8, 0x10ffa9, 0x10ffaa, 0x10ffab, 0x10ffac, 0x10ffad, 0x10ffae, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x7007a, 0xb07f8, 0x10ffaf, 0x10ffb0, 0x10ffb1, 0x10ffb2, 0x10ffb3, 0x10ffb4, 0x10ffb5, 0x10ffb6, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x800f9, 0x10ffb7, 0x10ffb8, 0x10ffb9, 0x10ffba, 0x10ffbb, 0x10ffbc, 0x10ffbd, 0x10ffbe, 0x10ffbf, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f7, 0x10ffc0, 0x10ffc1, 0x10ffc2, 0x10ffc3, 0x10ffc4, 0x10ffc5, 0x10ffc6, 0x10ffc7, 0x10ffc8, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f8, 0x10ffc9, 0x10ffca, 0x10ffcb, 0x10ffcc, 0x10ffcd, 0x10ffce, 0x10ffcf, 0x10ffd0, 0x10ffd1, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901f9, 0x10ffd2, 0x10ffd3, 0x10ffd4, 0x10ffd5, 0x10ffd6, 0x10ffd7, 0x10ffd8, 0x10ffd9, 0x10ffda, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0x901fa, 0x10ffdb, 0x10ffdc, 0x10ffdd, 0x10ffde, 0x10ffdf, 0x10ffe0, 0x10ffe1, 0x10ffe2, 0x10ffe3, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xb07f9, 0x10ffe4, 0x10ffe5, 0x10ffe6, 0x10ffe7, 0x10ffe8, 0x10ffe9, 0x10ffea, 0x10ffeb, 0x10ffec, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0x00000, 0xe3fe0, 0x10ffed, 0x10ffee, 0x10ffef, 0x10fff0, 0x10fff1, 0x10fff2, 0x10fff3, 0x10fff4, 0x10fff5, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
    0xa03fa, 0xf7fc3, 0x10fff6, 0x10fff7, 0x10fff8, 0x10fff9, 0x10fffa, 0x10fffb, 0x10fffc, 0x10fffd, 0x10fffe, 0x00000, 0x00000, 0x00000, 0x00000, 0x00000,
  },
};
// category -> length << 16 | code, tables K.3 and K.4
__device__ const unsigned JP_DC[2][12] = {
  {0x20000, 0x30002, 0x30003, 0x30004, 0x30005, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe},
  {0x20000, 0x20001, 0x20002, 0x30006, 0x4000e, 0x5001e, 0x6003e, 0x7007e, 0x800fe, 0x901fe, 0xa03fe, 0xb07fe},
};
__device__ const unsigned char JP_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// A call as the kernels see it, as kernel arguments: no allocation, no copy, no host wait.
struct JpTab {
  const uint8_t* rgb[JP_MAX_N];
  uint8_t* out[JP_MAX_N];
  long long cap[JP_MAX_N];
  unsigned short H[JP_MAX_N], W[JP_MAX_N];          // <= JP_MAX_DIM
  int blk0[JP_MAX_N + 1];                           // prefix of the pictures' block counts: coefficient, DC and offset arrays
  int bt0[JP_MAX_N + 1];                            // prefix of their block-tile counts
  int wt0[JP_MAX_N + 1];                            // prefix of their worst-case word-tile counts
  long long raw0[JP_MAX_N + 1];                     // prefix of their raw-stream bytes in the workspace (multiples of 4)
  int n, sub;                                       // sub: 444 or 420
};
struct JpQuant {
  unsigned short q[2][64];                          // luminance, chrominance; natural order
};
// the fattest launch: the table, the quantisation tables, three pointers and the runtime's 256 implicit bytes
static_assert(sizeof(JpTab) + sizeof(JpQuant) + 24 + 256 <= 4096, "the table and the other arguments of a launch must fit in 4 KB");

// the workspace, carved in one place
struct JpWs {
  unsigned long long *btoff, *ffoff, *info;         // [bt], [wt], [n]: tile bit offsets, tile stuffing offsets, bits per picture
  unsigned* raw;                                    // the unstuffed stream, one 32-bit word (first bit = bit 31) per entry
  short* coef;                                      // [blocks][64]
  unsigned* loc;                                    // [blocks]: AC bits after kernel 1, the block's bit offset in its tile after kernel 2
  unsigned *btsum, *fft;                            // [bt], [wt]
  short* dc;                                        // [blocks]
  size_t bytes;
};

// ---- arithmetic -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int jp_component(const uint8_t* __restrict__ p, int comp) {
  const int r = p[0], g = p[1], b = p[2];
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + 8388608 + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + 8388608 + 32767) >> 16;
}
__device__ __forceinline__ int jp_min(int a, int b) { return a < b ? a : b; }
struct alignas(16) JpWord4 {
  unsigned x, y, z, w;
};
__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of the Independent JPEG Group's accurate integer DCT over v[0], v[S], .. v[7 S]
template <bool ROWS, int S>
__device__ __forceinline__ void jp_dct8(int* v) {
  constexpr int n = ROWS ? 11 : 15;
  int t0 = v[0] + v[7 * S], t1 = v[S] + v[6 * S], t2 = v[2 * S] + v[5 * S], t3 = v[3 * S] + v[4 * S];
  int t7 = v[0] - v[7 * S], t6 = v[S] - v[6 * S], t5 = v[2 * S] - v[5 * S], t4 = v[3 * S] - v[4 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  v[0] = ROWS ? (t10 + t11) * 4 : jp_descale(t10 + t11, 2);
  v[4 * S] = ROWS ? (t10 - t11) * 4 : jp_descale(t10 - t11, 2);
  const int z = (t12 + t13) * 4433;
  v[2 * S] = jp_descale(z + t13 * 6270, n);
  v[6 * S] = jp_descale(z - t12 * 15137, n);
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  v[7 * S] = jp_descale(t4 + z1 + z3, n);
  v[5 * S] = jp_descale(t5 + z2 + z4, n);
  v[3 * S] = jp_descale(t6 + z2 + z3, n);
  v[S] = jp_descale(t7 + z1 + z4, n);
}

__device__ __forceinline__ int jp_bitlen(int v) { return 32 - __clz(v < 0 ? -v : v); }        // 0 for 0
__device__ __forceinline__ int jp_comp_of(int b, int sub) {
  if (sub == 444) return b % 3;
  const int k = b % 6;
  return k < 4 ? 0 : k - 3;
}
// the block coded before b in b's component; < 0: none
__device__ __forceinline__ int jp_prev_of(int b, int sub) {
  if (sub == 444) return b - 3;
  const int k = b % 6;
  return k == 0 ? b - 3 : (k < 4 ? b - 1 : b - 6);
}
// quantised DC of block b of a picture whose DC row is d: a dummy repeats the block before it (never the first of an MCU)
__device__ __forceinline__ int jp_dc_of(const short* __restrict__ d, int b) {
  int v = d[b];
  while (v == JP_DUMMY_DC) v = d[--b];
  return v;
}
__device__ __forceinline__ int jp_dc_diff(const short* __restrict__ d, int b, int sub) {
  const int p = jp_prev_of(b, sub);
  return jp_dc_of(d, b) - (p < 0 ? 0 : jp_dc_of(d, p));
}

// exclusive scan of one value per thread over the workgroup's 256 threads (every thread calls); *total: the sum
__device__ __forceinline__ unsigned jp_wg_scan(unsigned v, unsigned* total) {
  __shared__ unsigned s[256];
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const unsigned a = t >= d ? s[t - d] : 0u;
    __syncthreads();
    s[t] += a;
    __syncthreads();
  }
  const unsigned incl = s[t];
  *total = s[255];
  __syncthreads();
  return incl - v;
}

// sum of one value per thread over the workgroup's 256 threads (every thread calls): a butterfly inside each wave, then the four
// waves' sums through LDS - two barriers; the result is valid in thread 0
__device__ __forceinline__ unsigned jp_wg_sum(unsigned v) {
  __shared__ unsigned s[4];
  v += __shfl_xor(v, 32);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const unsigned total = s[0] + s[1] + s[2] + s[3];
  __syncthreads();
  return total;
}

// ---- 1: transform -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_transform_kernel(JpTab T, JpQuant Q, short* __restrict__ coef, short* __restrict__ dc,
                                                             unsigned* __restrict__ acbits) {
  __shared__ unsigned char s_len[2][256];                       // AC code lengths
  for (int i = threadIdx.x; i < 512; i += 256) s_len[i >> 8][i & 255] = (unsigned char)(JP_AC[i >> 8][i & 255] >> 16);
  __syncthreads();
  const int pic = blockIdx.y;
  const int g0 = T.blk0[pic], nblk = T.blk0[pic + 1] - g0;
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= nblk) return;
  const int H = T.H[pic], W = T.W[pic];
  const uint8_t* __restrict__ rgb = T.rgb[pic];
  short* __restrict__ out = coef + ((size_t)g0 + b) * 64;
  int v[64];
  int comp;
  if (T.sub == 444) {
    const int bw = (W + 7) >> 3, mcu = b / 3;
    comp = b - 3 * mcu;
    const int by = mcu / bw, bx = mcu - by * bw;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int y = jp_min(by * 8 + r, H - 1);
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int x = jp_min(bx * 8 + c, W - 1);
        v[8 * r + c] = jp_component(rgb + ((size_t)y * W + x) * 3, comp) - 128;
      }
    }
  } else {
    const int mw = (W + 15) >> 4, mcu = b / 6, k = b - 6 * mcu;
    const int my = mcu / mw, mx = mcu - my * mw;
    comp = k < 4 ? 0 : k - 3;
    if (k < 4) {
      const int by = 2 * my + (k >> 1), bx = 2 * mx + (k & 1);
      if (by >= ((H + 7) >> 3) || bx >= ((W + 7) >> 3)) {          // a dummy block: not transformed
        JpWord4* o4 = reinterpret_cast<JpWord4*>(out);
#pragma unroll
        for (int i = 0; i < 8; ++i) o4[i] = JpWord4{0u, 0u, 0u, 0u};
        dc[g0 + b] = JP_DUMMY_DC;
        acbits[g0 + b] = s_len[0][0];                              // end-of-block alone
        return;
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int y = jp_min(by * 8 + r, H - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int x = jp_min(bx * 8 + c, W - 1);
          v[8 * r + c] = jp_component(rgb + ((size_t)y * W + x) * 3, 0) - 128;
        }
      }
    } else {
      // the downsampled plane has ceil(H / 2) rows (one repeated input row under an odd H) and repeats its own last row below;
      // to the right the INPUT's last column repeats
      const int ch = (H + 1) >> 1;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int cy = jp_min(my * 8 + r, ch - 1);
        const int y0 = 2 * cy, y1 = jp_min(2 * cy + 1, H - 1);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int cx = mx * 8 + c;
          const int x0 = jp_min(2 * cx, W - 1), x1 = jp_min(2 * cx + 1, W - 1);
          const int s = jp_component(rgb + ((size_t)y0 * W + x0) * 3, comp) + jp_component(rgb + ((size_t)y0 * W + x1) * 3, comp) +
                        jp_component(rgb + ((size_t)y1 * W + x0) * 3, comp) + jp_component(rgb + ((size_t)y1 * W + x1) * 3, comp);
          v[8 * r + c] = ((s + 1 + (c & 1)) >> 2) - 128;           // mx * 8 is even: the column's parity is c's
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) jp_dct8<true, 1>(v + 8 * r);
#pragma unroll
  for (int c = 0; c < 8; ++c) jp_dct8<false, 8>(v + c);
  const int t = comp == 0 ? 0 : 1;
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    const unsigned d = 8u * (t == 0 ? Q.q[0][i] : Q.q[1][i]);
    const unsigned a = (unsigned)(v[i] < 0 ? -v[i] : v[i]);
    const int q = (int)((a + (d >> 1)) / d);
    v[i] = v[i] < 0 ? -q : q;
  }
  unsigned bits = 0;
  int run = 0;
  unsigned w[32];
#pragma unroll
  for (int k = 0; k < 64; ++k) {
    const int c = v[JP_ZZ[k]];
    if (k & 1) w[k >> 1] |= (unsigned)(c & 0xffff) << 16; else w[k >> 1] = (unsigned)(c & 0xffff);
    if (k == 0) continue;
    if (c == 0) {
      ++run;
    } else {
      bits += (unsigned)(run >> 4) * s_len[t][0xF0];
      const int size = jp_bitlen(c);
      bits += s_len[t][((run & 15) << 4) | size] + size;
      run = 0;
    }
  }
  if (run) bits += s_len[t][0];
  JpWord4* o4 = reinterpret_cast<JpWord4*>(out);
#pragma unroll
  for (int i = 0; i < 8; ++i) o4[i] = JpWord4{w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]};
  dc[g0 + b] = (short)v[0];
  acbits[g0 + b] = bits;
}

// ---- 2: bits per block, scanned inside a tile -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_bits_kernel(JpTab T, const short* __restrict__ dc, unsigned* __restrict__ loc,
                                                        unsigned* __restrict__ btsum) {
  const int pic = blockIdx.y;
  const int g0 = T.blk0[pic], nblk = T.blk0[pic + 1] - g0;
  const int base = blockIdx.x * JP_TILE_BLOCKS;
  if (base >= nblk) return;                                        // the whole workgroup
  const short* __restrict__ d = dc + g0;
  unsigned bits[4], sum = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = base + threadIdx.x * 4 + j;
    bits[j] = 0;
    if (b < nblk) {
      const int cat = jp_bitlen(jp_dc_diff(d, b, T.sub));
      bits[j] = loc[g0 + b] + (JP_DC[jp_comp_of(b, T.sub) ? 1 : 0][cat] >> 16) + cat;
    }
    sum += bits[j];
  }
  unsigned total;
  unsigned at = jp_wg_scan(sum, &total);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int b = base + threadIdx.x * 4 + j;
    if (b < nblk) loc[g0 + b] = at;
    at += bits[j];
  }
  if (threadIdx.x == 0) btsum[T.bt0[pic] + blockIdx.x] = total;
}

// ---- 3 and 5: per picture, the exclusive prefix of its tiles' sums ---------------------------------------------------------------
// mode 0: block tiles -> info[pic] = the picture's bits.  mode 1: word tiles (those that hold bytes) -> lengths[pic].
// A tile sums to less than 2^21 (1024 blocks x 1660 bits; 1024 bytes), a picture to more than 2^32 bits at the size limit: 64-bit offsets.
__global__ __launch_bounds__(256) void jpeg_scan_kernel(JpTab T, int mode, const unsigned* __restrict__ sums,
                                                        unsigned long long* __restrict__ offs, unsigned long long* __restrict__ info,
                                                        long long* __restrict__ lengths) {
  const int pic = blockIdx.x;
  const int nblk = T.blk0[pic + 1] - T.blk0[pic];
  long long nbytes = 0;
  int base, cnt;
  if (mode == 0) {
    base = T.bt0[pic];
    cnt = (nblk + JP_TILE_BLOCKS - 1) / JP_TILE_BLOCKS;
  } else {
    base = T.wt0[pic];
    nbytes = (long long)((info[pic] + 7) >> 3);
    cnt = (int)((nbytes + 4 * JP_TILE_WORDS - 1) / (4 * JP_TILE_WORDS));
  }
  unsigned long long carry = 0;
  for (int c0 = 0; c0 < cnt; c0 += 256) {
    const int i = c0 + threadIdx.x;
    unsigned total;
    const unsigned e = jp_wg_scan(i < cnt ? sums[base + i] : 0u, &total);
    if (i < cnt) offs[base + i] = carry + e;
    carry += total;
  }
  if (threadIdx.x == 0) {
    if (mode == 0) info[pic] = carry; else lengths[pic] = nbytes + (long long)carry;
  }
}

// ---- 4: one thread per stream word ------------------------------------------------------------------------------------------------
// `at` is the position of the next code relative to the word's first bit; a code of `len` bits lands in the word where it overlaps
// [0, 32).  The shift drops what lies before the word (the high bits of a 32-bit left shift) or behind it (a right shift).
__device__ __forceinline__ void jp_put(unsigned& word, int& at, unsigned code, int len) {
  if (len > 0 && at + len > 0 && at < 32) {
    const int sh = 32 - at - len;
    word |= sh >= 0 ? code << sh : code >> -sh;
  }
  at += len;
}
__device__ __forceinline__ unsigned jp_value_bits(int v, int size) { return (unsigned)(v < 0 ? v - 1 : v) & ((1u << size) - 1u); }
__device__ __forceinline__ unsigned jp_count_ff(unsigned word, int nvalid) {
  unsigned n = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) n += (j < nvalid && ((word >> (24 - 8 * j)) & 255u) == 255u) ? 1u : 0u;
  return n;
}

__global__ __launch_bounds__(256) void jpeg_emit_kernel(JpTab T, const short* __restrict__ coef, const short* __restrict__ dc,
                                                        const unsigned* __restrict__ loc, const unsigned long long* __restrict__ btoff,
                                                        const unsigned long long* __restrict__ info, unsigned* __restrict__ raw,
                                                        unsigned* __restrict__ fft) {
  const int pic = blockIdx.y;
  const unsigned long long bits = info[pic];
  if ((unsigned long long)blockIdx.x * (32 * JP_TILE_WORDS) >= bits) return;       // the whole workgroup: no word of this tile exists
  __shared__ unsigned s_ac[2][256];
  for (int i = threadIdx.x; i < 512; i += 256) s_ac[i >> 8][i & 255] = JP_AC[i >> 8][i & 255];
  __syncthreads();
  const int g0 = T.blk0[pic], nblk = T.blk0[pic + 1] - g0, sub = T.sub;
  const long long nbytes = (long long)((bits + 7) >> 3);
  const long long w = (long long)blockIdx.x * JP_TILE_WORDS + threadIdx.x;
  unsigned word = 0, nff = 0;
  if (4 * w < nbytes) {
    const unsigned long long p0 = 32ull * (unsigned long long)w;
    // the block that holds bit p0: the last tile, then the last block of it, that starts at or before p0 (every block has bits)
    const unsigned long long* __restrict__ to = btoff + T.bt0[pic];
    int lo = 0, hi = (nblk + JP_TILE_BLOCKS - 1) / JP_TILE_BLOCKS;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (to[mid] <= p0) lo = mid; else hi = mid;
    }
    const unsigned long long t0 = to[lo];
    const unsigned rel = (unsigned)(p0 - t0);
    const unsigned* __restrict__ lc = loc + g0;
    int b = lo * JP_TILE_BLOCKS;
    hi = jp_min(nblk, b + JP_TILE_BLOCKS);
    while (hi - b > 1) {
      const int mid = (b + hi) >> 1;
      if (lc[mid] <= rel) b = mid; else hi = mid;
    }
    int at = (int)((long long)lc[b] - (long long)rel);              // <= 0
    const short* __restrict__ d = dc + g0;
    while (at < 32 && b < nblk) {
      const int t = jp_comp_of(b, sub) ? 1 : 0;
      const int diff = jp_dc_diff(d, b, sub);
      const int cat = jp_bitlen(diff);
      const unsigned e = JP_DC[t][cat];
      jp_put(word, at, ((e & 0xffffu) << cat) | jp_value_bits(diff, cat), (int)(e >> 16) + cat);
      const short* __restrict__ c = coef + ((size_t)g0 + b) * 64;
      int run = 0, k = 1;
      for (; k < 64 && at < 32; ++k) {
        const int v = c[k];
        if (v == 0) { ++run; continue; }
        for (; run >= 16; run -= 16) jp_put(word, at, s_ac[t][0xF0] & 0xffffu, (int)(s_ac[t][0xF0] >> 16));
        const int size = jp_bitlen(v);
        const unsigned a = s_ac[t][(run << 4) | size];
        jp_put(word, at, ((a & 0xffffu) << size) | jp_value_bits(v, size), (int)(a >> 16) + size);
        run = 0;
      }
      if (k == 64 && run) jp_put(word, at, s_ac[t][0] & 0xffffu, (int)(s_ac[t][0] >> 16));
      ++b;
    }
    if (b == nblk && at < 32) {                                     // the last byte is filled with 1-bits
      const int pad = (int)(8ull * (unsigned long long)nbytes - bits);
      jp_put(word, at, (1u << pad) - 1u, pad);
    }
    const int nvalid = (int)(nbytes - 4 * w < 4 ? nbytes - 4 * w : 4);
    nff = jp_count_ff(word, nvalid);
    const long long rawcap = T.raw0[pic + 1] - T.raw0[pic];
    if (4 * w + 4 <= rawcap) raw[T.raw0[pic] / 4 + w] = word;
  }
  const unsigned total = jp_wg_sum(nff);
  if (threadIdx.x == 0) fft[T.wt0[pic] + blockIdx.x] = total;
}

// ---- 6: byte stuffing -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void jpeg_stuff_kernel(JpTab T, const unsigned* __restrict__ raw,
                                                         const unsigned long long* __restrict__ ffoff,
                                                         const unsigned long long* __restrict__ info) {
  const int pic = blockIdx.y;
  const long long nbytes = (long long)((info[pic] + 7) >> 3);
  const long long rawcap = T.raw0[pic + 1] - T.raw0[pic];
  const long long first = (long long)blockIdx.x * (4 * JP_TILE_WORDS);
  if (first >= nbytes || first >= rawcap) return;                   // the whole workgroup
  const long long w = (long long)blockIdx.x * JP_TILE_WORDS + threadIdx.x;
  const bool have = 4 * w < nbytes && 4 * w + 4 <= rawcap;
  const unsigned word = have ? raw[T.raw0[pic] / 4 + w] : 0u;
  const int nvalid = have ? (int)(nbytes - 4 * w < 4 ? nbytes - 4 * w : 4) : 0;
  unsigned total;
  const unsigned before = jp_wg_scan(jp_count_ff(word, nvalid), &total);
  if (!have) return;
  long long pos = 4 * w + (long long)ffoff[T.wt0[pic] + blockIdx.x] + before;
  const long long cap = T.cap[pic];
  uint8_t* __restrict__ out = T.out[pic];
  for (int j = 0; j < nvalid; ++j) {
    const unsigned byte = (word >> (24 - 8 * j)) & 255u;
    if (pos < cap) out[pos] = (uint8_t)byte;
    ++pos;
    if (byte == 255u) {
      if (pos < cap) out[pos] = 0;
      ++pos;
    }
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
static void jp_quant_tables(int quality, JpQuant* Q) {
  static const unsigned char base[2][64] = {
      {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
       14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
      {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
       99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
  const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      int q = (base[t][i] * s + 50) / 100;
      q = q < 1 ? 1 : (q > 255 ? 255 : q);
      Q->q[t][i] = (unsigned short)q;
    }
}

static int jp_blocks(int H, int W, int sub) {
  return sub == 444 ? 3 * ((H + 7) / 8) * ((W + 7) / 8) : 6 * ((H + 15) / 16) * ((W + 15) / 16);
}

// checks the table's sizes and fills the prefixes
static int jp_table(const dyb_jpeg_desc* desc, int N, int sub, JpTab* T) {
  DYB_REQUIRE(desc && N >= 1, DYB_ERR_ARG);
  for (int i = 0; i < (N < JP_MAX_N ? N : JP_MAX_N); ++i) DYB_REQUIRE(desc[i].H >= 1 && desc[i].W >= 1 && desc[i].capacity >= 0, DYB_ERR_ARG);
  DYB_REQUIRE(N <= JP_MAX_N && (sub == 444 || sub == 420), DYB_ERR_UNSUPPORTED);
  T->n = N;
  T->sub = sub;
  T->blk0[0] = T->bt0[0] = T->wt0[0] = 0;
  T->raw0[0] = 0;
  for (int i = 0; i < N; ++i) {
    DYB_REQUIRE(desc[i].H <= JP_MAX_DIM && desc[i].W <= JP_MAX_DIM, DYB_ERR_UNSUPPORTED);
    const int nblk = jp_blocks(desc[i].H, desc[i].W, sub);
    const long long words = (long long)nblk * JP_BLOCK_WORDS;
    const long long capw = (desc[i].capacity + 3) / 4;
    T->H[i] = (unsigned short)desc[i].H;
    T->W[i] = (unsigned short)desc[i].W;
    T->blk0[i + 1] = T->blk0[i] + nblk;                              // 64 pictures of 3 x 1024 x 1024 blocks: 2e8
    T->bt0[i + 1] = T->bt0[i] + (nblk + JP_TILE_BLOCKS - 1) / JP_TILE_BLOCKS;
    T->wt0[i + 1] = T->wt0[i] + (int)((words + JP_TILE_WORDS - 1) / JP_TILE_WORDS);      // 64 x 6.4e5
    T->raw0[i + 1] = T->raw0[i] + 4 * (capw < words ? capw : words);
  }
  return DYB_OK;
}

static void jp_carve(const JpTab& T, void* ws, JpWs* L) {
  const size_t nblk = (size_t)T.blk0[T.n], bt = (size_t)T.bt0[T.n], wt = (size_t)T.wt0[T.n];
  char* p = reinterpret_cast<char*>(((uintptr_t)ws + 15) & ~(uintptr_t)15);
  char* const p0 = p;
  auto take = [&](size_t bytes) { char* r = p; p += (bytes + 15) & ~(size_t)15; return r; };
  L->btoff = reinterpret_cast<unsigned long long*>(take(bt * 8));
  L->ffoff = reinterpret_cast<unsigned long long*>(take(wt * 8));
  L->info = reinterpret_cast<unsigned long long*>(take((size_t)T.n * 8));
  L->raw = reinterpret_cast<unsigned*>(take((size_t)T.raw0[T.n]));
  L->coef = reinterpret_cast<short*>(take(nblk * 128));
  L->loc = reinterpret_cast<unsigned*>(take(nblk * 4));
  L->btsum = reinterpret_cast<unsigned*>(take(bt * 4));
  L->fft = reinterpret_cast<unsigned*>(take(wt * 4));
  L->dc = reinterpret_cast<short*>(take(nblk * 2));
  L->bytes = (size_t)(p - p0) + 16;                                  // + the alignment of ws itself
}

extern "C" size_t dyb_jpeg_workspace_bytes(const dyb_jpeg_desc* desc, int N, int subsampling) {
  JpTab T;
  if (jp_table(desc, N, subsampling, &T) != DYB_OK) return 0;
  JpWs L;
  jp_carve(T, nullptr, &L);
  return L.bytes;
}

extern "C" int dyb_jpeg_encode_many(const dyb_jpeg_desc* desc, int N, int quality, int subsampling, long long* lengths, void* ws,
                                    size_t ws_bytes, hipStream_t st) {
  JpTab T;
  DYB_REQUIRE(lengths && quality >= 1 && quality <= 100, DYB_ERR_ARG);
  const int rc = jp_table(desc, N, subsampling, &T);
  if (rc != DYB_OK) return rc;
  for (int i = 0; i < N; ++i) {
    DYB_REQUIRE(desc[i].rgb && desc[i].out, DYB_ERR_ARG);
    T.rgb[i] = desc[i].rgb;
    T.out[i] = desc[i].out;
    T.cap[i] = desc[i].capacity;
  }
  JpWs L;
  jp_carve(T, ws, &L);
  DYB_REQUIRE(ws && ws_bytes >= L.bytes, DYB_ERR_WORKSPACE);
  JpQuant Q;
  jp_quant_tables(quality, &Q);
  int max_blk = 0, max_wt = 0;
  long long max_raw = 0;
  for (int i = 0; i < N; ++i) {
    max_blk = std::max(max_blk, T.blk0[i + 1] - T.blk0[i]);
    max_wt = std::max(max_wt, T.wt0[i + 1] - T.wt0[i]);
    max_raw = std::max(max_raw, T.raw0[i + 1] - T.raw0[i]);
  }
  const unsigned n = (unsigned)N;
  hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)dyb_cdiv(max_blk, 256), n), dim3(256), 0, st, T, Q, L.coef, L.dc, L.loc);
  DYB_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_bits_kernel, dim3((unsigned)dyb_cdiv(max_blk, JP_TILE_BLOCKS), n), dim3(256), 0, st, T, L.dc, L.loc, L.btsum);
  DYB_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n), dim3(256), 0, st, T, 0, L.btsum, L.btoff, L.info, lengths);
  DYB_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_emit_kernel, dim3((unsigned)max_wt, n), dim3(256), 0, st, T, L.coef, L.dc, L.loc, L.btoff, L.info, L.raw, L.fft);
  DYB_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3(n), dim3(256), 0, st, T, 1, L.fft, L.ffoff, L.info, lengths);
  DYB_CHECK_LAUNCH();
  const long long stuff_tiles = (max_raw + 4 * JP_TILE_WORDS - 1) / (4 * JP_TILE_WORDS);
  if (stuff_tiles > 0) {
    hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((unsigned)stuff_tiles, n), dim3(256), 0, st, T, L.raw, L.ffoff, L.info);
    DYB_CHECK_LAUNCH();
  }
  return DYB_OK;
}
