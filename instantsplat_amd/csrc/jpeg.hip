// Baseline JPEG encoding of 8-bit RGB frames on the device (include/mi355gs.h, mi355gs_jpeg_rgb8): libjpeg's integer colour
// conversion, edge padding, 2x2 chroma downsampling, `islow` forward DCT and quantisation, the typical Huffman tables of Annex K.3
// and one restart interval per MCU row — the file PIL (libjpeg-turbo) writes with optimize=False, restart_marker_rows=1, byte
// for byte (tests/jpeg_util.py restates it on the host).  All arithmetic is integer: nothing depends on contraction flags.
//
// An MCU row is a restart interval: it starts on a byte with its predictors at 0, so it is coded by one workgroup on its own.
// Its length is known only once its bits are laid out (a zero follows every FF byte, which depends on the byte alignment), so:
//
// Three launches whatever N is:
//   k_jpeg_rows<false> (MCU rows, N):     transform + quantise, the coefficients to scratch, the interval packed in LDS and counted
//   k_jpeg_scan        (1):               interval positions, file offsets
//   k_jpeg_rows<true>  (MCU rows + 1, N): the coefficients back from scratch, packed again and stored at their final place; the
//                                         extra workgroup of a frame writes the header and EOI.  A file that would reach past
//                                         out_bytes is not written at all.
// An interval is packed in groups of JPG_GROUP blocks (whole MCUs) with a carried bit position: the staging holds a group's worst
// case (JPG_BLOCK_BITS per block), whatever the content.
#include "common.h"
#include <string.h>
#include <initializer_list>

namespace {

constexpr int JPG_T = 256;               // threads of every workgroup here
constexpr int JPG_GROUP = 252;           // blocks packed per round: whole MCUs of 3 (4:4:4) and of 6 (4:2:0) blocks
constexpr int JPG_BLOCK_BITS = 1660;     // a block's code at most: DC 11 + 11 bits, 63 x (16 + 10)
constexpr int JPG_STAGE_WORDS = (7 + JPG_GROUP * JPG_BLOCK_BITS + 7 + 31) / 32 + 2;   // carried bits + a group + the padding
constexpr int JPG_CW = 33;               // 32-bit words per block of coefficients in LDS (64 int16 + 1 word: odd, conflict-free)
constexpr int JPG_HDR = 629;             // bytes of a file in front of its entropy-coded data
static_assert(JPG_GROUP % 6 == 0 && JPG_GROUP <= JPG_T, "a group is whole MCUs, one block per thread");

struct JpgLayout {
  bool ok = false;
  int sub = 0, mcu = 8, bpm = 3;               // MCU edge in pixels, blocks per MCU
  int mcols = 0, mrows = 0, nb = 0;            // MCUs per MCU row, MCU rows (= restart intervals), blocks per interval
  size_t coef = 0, meta = 0, rel = 0, total = 0;   // offsets into scratch
  size_t file_max = 0;
  __host__ JpgLayout(int N, int H, int W, int sub_) {
    if (N <= 0 || H <= 0 || W <= 0 || N > 65535 || H > 65535 || W > 65535 || (sub_ != 0 && sub_ != 2)) return;
    if (3LL * H * W > 0x7fffffffLL) return;
    sub = sub_; mcu = sub ? 16 : 8; bpm = sub ? 6 : 3;
    mcols = (W + mcu - 1) / mcu; mrows = (H + mcu - 1) / mcu; nb = mcols * bpm;
    const size_t S = (size_t)N * mrows;
    size_t o = 0;
    coef = o; o += gs_align(S * nb * 64 * sizeof(int16_t));   // per interval: its blocks' quantised coefficients, zigzag order
    meta = o; o += gs_align(S * sizeof(uint32_t));            // per interval: bytes of its entropy-coded data
    rel = o; o += gs_align(S * sizeof(int64_t));              // per interval: its position (marker included) behind the header
    total = o;
    const size_t interval_max = 2 * (((size_t)nb * JPG_BLOCK_BITS + 7) / 8);   // every byte an FF
    file_max = JPG_HDR + (size_t)mrows * interval_max + 2 * (size_t)(mrows - 1) + 2;
    ok = true;
  }
};

constexpr uint8_t JPG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---- the typical Huffman tables of the JPEG standard, Annex K.3: counts per code length, then the values
constexpr uint8_t JPG_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t JPG_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
constexpr uint8_t JPG_AC_VALS[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// the canonical codes (Annex C) as code | length << 16, indexed by value; [0], [1]: DC luma, chroma; [2], [3]: AC luma, chroma
struct JpgCodes { uint32_t v[4][256]; };
constexpr JpgCodes jpg_make_codes() {
  JpgCodes c{};
  for (int tab = 0; tab < 4; ++tab) {
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
      const int cnt = tab < 2 ? JPG_DC_BITS[tab][l - 1] : JPG_AC_BITS[tab - 2][l - 1];
      for (int i = 0; i < cnt; ++i, ++k, ++code) c.v[tab][tab < 2 ? k : JPG_AC_VALS[tab - 2][k]] = code | ((uint32_t)l << 16);
      code <<= 1;
    }
  }
  return c;
}
__device__ const JpgCodes k_jpg_codes = jpg_make_codes();

struct JpgQuant { uint8_t q[2][64]; };          // natural order, 1..255
struct JpgHeader { uint8_t b[JPG_HDR + 3]; };   // built by the host per call
struct JpgGeom { int H, W, sub, bpm, mcols, mrows, nb; };

// ---- libjpeg jfdctint.c (islow): one pass over 8 values.  FIRST: pass 1 (rows; results scaled up by 4), else pass 2 (columns)
template <bool FIRST>
__device__ __forceinline__ void jpg_dct8(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
  constexpr int n = FIRST ? 11 : 15, half = 1 << (n - 1);
  int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d0 = FIRST ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
  d4 = FIRST ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
  const int z = (t12 + t13) * 4433;
  d2 = (z + t13 * 6270 + half) >> n;
  d6 = (z - t12 * 15137 + half) >> n;
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  d7 = (t4 + z1 + z3 + half) >> n;
  d5 = (t5 + z2 + z4 + half) >> n;
  d3 = (t6 + z2 + z3 + half) >> n;
  d1 = (t7 + z1 + z4 + half) >> n;
}

// component c (0: Y, 1: Cb, 2: Cr) of one pixel: libjpeg's 16-bit fixed point (jccolor.c)
__device__ __forceinline__ int jpg_ycc(const uint8_t* __restrict__ p, int c) {
  const int r = p[0], g = p[1], b = p[2];
  return c == 0 ? (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
       : c == 1 ? (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
                : (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// One 8x8 block — component `comp`, block row `by`, block column `bx` of the component's plane — from the frame to its 64
// quantised coefficients in zigzag order, two per word.  `half`: the component is downsampled 2x2 (chroma at 4:2:0).
// Edges as libjpeg has them: a full-resolution plane repeats its last column and row; a downsampled plane averages
// (a00 + a01 + a10 + a11 + bias) >> 2, bias 1, 2, 1, 2, ... along a row, over a source that repeats its last column and has its
// last row repeated to an even count only — below that the DOWNSAMPLED plane repeats its last row.
// dc_only: a dummy block (its DC from this block, no AC).
__device__ void jpg_block(const uint8_t* __restrict__ img, int H, int W, int comp, bool half, int by, int bx,
                          const uint32_t* __restrict__ q8tab, bool dc_only, uint32_t* __restrict__ dst) {
  int ws[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int s[8];
    if (!half) {
      const int y = min(by * 8 + i, H - 1);
#pragma unroll
      for (int j = 0; j < 8; ++j) s[j] = jpg_ycc(img + ((size_t)y * W + min(bx * 8 + j, W - 1)) * 3, comp) - 128;
    } else {
      const int cy = min(by * 8 + i, (H + 1) / 2 - 1);
      const uint8_t* r0 = img + (size_t)(2 * cy) * W * 3;
      const uint8_t* r1 = img + (size_t)min(2 * cy + 1, H - 1) * W * 3;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int x0 = min(2 * (bx * 8 + j), W - 1) * 3, x1 = min(2 * (bx * 8 + j) + 1, W - 1) * 3;
        s[j] = ((jpg_ycc(r0 + x0, comp) + jpg_ycc(r0 + x1, comp) + jpg_ycc(r1 + x0, comp) + jpg_ycc(r1 + x1, comp) + 1 + (j & 1)) >> 2) - 128;
      }
    }
    jpg_dct8<true>(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7]);
#pragma unroll
    for (int j = 0; j < 8; ++j) ws[i * 8 + j] = s[j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
    jpg_dct8<false>(ws[j], ws[8 + j], ws[16 + j], ws[24 + j], ws[32 + j], ws[40 + j], ws[48 + j], ws[56 + j]);
#pragma unroll
  for (int k = 0; k < 64; k += 2) {
    uint32_t word = 0;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int nat = JPG_ZIGZAG[k + e];
      const int c = ws[nat];
      const uint32_t q8 = q8tab[nat];   // 8 q: the transform's results are 8 x the DCT
      const int v = (int)(((uint32_t)abs(c) + (q8 >> 1)) / q8);   // |c| < 2^15: the quotient fits 16 bits with its sign
      const int sv = (dc_only && k + e > 0) ? 0 : (c < 0 ? -v : v);
      word |= ((uint32_t)sv & 0xffffu) << (16 * e);
    }
    dst[k >> 1] = word;
  }
}

// MSB-first bit sink over 32-bit staging words (word w holds stream bits 32 w .. 32 w + 31, the first in bit 31)
struct JpgBits {
  uint32_t* stage;
  uint64_t acc;
  uint32_t fill, wi;
  __device__ __forceinline__ void put(uint32_t v, uint32_t n) {   // n <= 32, v < 2^n
    acc = (acc << n) | v;
    fill += n;
    if (fill >= 32) {
      fill -= 32;
      atomicOr(&stage[wi++], (uint32_t)(acc >> fill));
      acc &= (1ull << fill) - 1;
    }
  }
  __device__ __forceinline__ void flush() { if (fill) atomicOr(&stage[wi], (uint32_t)(acc << (32 - fill))); }
};

// the Huffman code of one block (its coefficients in `row`, the DC's prediction in `pred`): EMIT puts the bits, else only their
// number is returned
template <bool EMIT>
__device__ __forceinline__ uint32_t jpg_code_block(const uint32_t* __restrict__ row, int pred, const uint32_t* __restrict__ dc_tab,
                                                   const uint32_t* __restrict__ ac_tab, JpgBits& sink) {
  uint32_t bits = 0;
  auto code = [&](uint32_t cl, int v, uint32_t n) {   // the code of a symbol, then the low n bits of v (v - 1 for v < 0)
    const uint32_t len = (cl >> 16) + n;
    if (EMIT) sink.put(((cl & 0xffffu) << n) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u)), len);
    bits += len;
  };
  const int d = (int)(int16_t)(row[0] & 0xffffu) - pred;
  const uint32_t nd = d ? 32u - (uint32_t)__clz(abs(d)) : 0u;
  code(dc_tab[nd], d, nd);
  uint32_t run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = (int)(int16_t)((row[k >> 1] >> (16 * (k & 1))) & 0xffffu);
    if (v == 0) { ++run; continue; }
    for (; run >= 16; run -= 16) code(ac_tab[0xF0], 0, 0);
    const uint32_t n = 32u - (uint32_t)__clz(abs(v));
    code(ac_tab[((run << 4) | n) & 255u], v, n);
    run = 0;
  }
  if (run) code(ac_tab[0], 0, 0);
  return bits;
}

// One workgroup per (MCU row, frame).  EMIT false: transform, leave the coefficients in scratch and the interval's byte count in
// meta.  EMIT true: read the coefficients back and store the interval (behind its RST marker) at its place in the file;
// workgroup (MCU rows, frame) stores the header and EOI.
template <bool EMIT>
__global__ __launch_bounds__(JPG_T) void k_jpeg_rows(JpgGeom g, JpgQuant qt, const uint8_t* __restrict__ frames, uint32_t* __restrict__ coef,
                                                     uint32_t* __restrict__ meta, const int64_t* __restrict__ rel,
                                                     const int64_t* __restrict__ offsets, uint8_t* __restrict__ out, size_t out_bytes,
                                                     JpgHeader hdr) {
  __shared__ uint32_t s_coef[JPG_GROUP * JPG_CW];
  __shared__ uint32_t s_stage[JPG_STAGE_WORDS];
  __shared__ uint32_t s_tab[4][256];
  __shared__ uint32_t s_wbits[JPG_T / 64], s_wff[JPG_T / 64];
  __shared__ int s_pred[3];
  __shared__ uint32_t s_q8[2][64];

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int r = blockIdx.x, f = blockIdx.y;
  uint8_t* dst = nullptr;
  if (EMIT) {
    if ((unsigned long long)offsets[f + 1] > (unsigned long long)out_bytes) return;   // the file does not fit: none of it is written
    uint8_t* file = out + offsets[f];
    if (r == g.mrows) {
      for (int i = t; i < JPG_HDR; i += JPG_T) file[i] = hdr.b[i];
      if (t < 2) out[offsets[f + 1] - 2 + t] = t ? 0xD9 : 0xFF;
      return;
    }
    dst = file + JPG_HDR + rel[(size_t)f * g.mrows + r];
    if (r > 0) {
      if (t < 2) dst[t] = t ? (uint8_t)(0xD0 + ((r - 1) & 7)) : (uint8_t)0xFF;
      dst += 2;
    }
  }
  for (int i = t; i < 4 * 256; i += JPG_T) (&s_tab[0][0])[i] = (&k_jpg_codes.v[0][0])[i];
  for (int i = t; i < JPG_STAGE_WORDS; i += JPG_T) s_stage[i] = 0;
  if (t < 3) s_pred[t] = 0;
  if (!EMIT && t < 128) s_q8[t >> 6][t & 63] = (uint32_t)qt.q[t >> 6][t & 63] << 3;

  const uint8_t* img = frames + (size_t)f * (size_t)g.H * (size_t)g.W * 3;
  uint32_t* icoef = coef + ((size_t)f * g.mrows + r) * (size_t)g.nb * 32;
  const int ybh = (g.H + 7) >> 3, ybw = (g.W + 7) >> 3;   // blocks of the Y plane
  uint32_t carry = 0;      // bits of the open byte, in front of the staging
  uint32_t nout = 0;       // bytes of the interval so far
  for (int g0 = 0; g0 < g.nb; g0 += JPG_GROUP) {
    const int cnt = min(JPG_GROUP, g.nb - g0);
    __syncthreads();
    // ---- 1. the group's coefficients into LDS
    if (!EMIT) {
      if (t < cnt) {
        const int b = g0 + t, m = b / g.bpm, j = b - m * g.bpm;
        int comp = j, by = r, bx = m;
        bool half = false, dummy = false;
        if (g.sub) {
          if (j < 4) {
            // Y (0,0) (0,1) (1,0) (1,1): a block outside the plane is a dummy block — no AC, the DC of the block coded just
            // before it in the MCU, which is at the end of that chain the last real one (block 0 always is)
            int jj = j;
            while (2 * r + (jj >> 1) >= ybh || 2 * m + (jj & 1) >= ybw) --jj;
            dummy = jj != j;
            comp = 0; by = 2 * r + (jj >> 1); bx = 2 * m + (jj & 1);
          } else {
            comp = j - 3; half = true;
          }
        }
        jpg_block(img, g.H, g.W, comp, half, by, bx, s_q8[comp > 0], dummy, s_coef + t * JPG_CW);
      }
      __syncthreads();
      for (int i = t; i < cnt * 32; i += JPG_T) icoef[(size_t)g0 * 32 + i] = s_coef[(i >> 5) * JPG_CW + (i & 31)];
    } else {
      for (int i = t; i < cnt * 32; i += JPG_T) s_coef[(i >> 5) * JPG_CW + (i & 31)] = icoef[(size_t)g0 * 32 + i];
      __syncthreads();
    }
    // ---- 2. every block's bits, their positions by a workgroup scan, the codes into the staging words
    const bool act = t < cnt;
    const int j = act ? (g0 + t) % g.bpm : 0;
    const int comp = g.sub ? (j < 4 ? 0 : j - 3) : j;
    const int back = g.sub ? (j == 0 ? 3 : j < 4 ? 1 : 6) : 3;   // the component's previous block in coding order
    const uint32_t* row = s_coef + (act ? t : 0) * JPG_CW;
    const int pred = t >= back ? (int)(int16_t)(s_coef[(act ? t - back : 0) * JPG_CW] & 0xffffu) : s_pred[comp];
    const uint32_t* dc_tab = s_tab[comp > 0];
    const uint32_t* ac_tab = s_tab[2 + (comp > 0)];
    JpgBits sink{s_stage, 0, 0, 0};
    const uint32_t bits = act ? jpg_code_block<false>(row, pred, dc_tab, ac_tab, sink) : 0u;
    const uint32_t incl = gs_wave_scan_incl_u32(bits);
    if (lane == 63) s_wbits[wv] = incl;
    __syncthreads();
    uint32_t off = carry + incl - bits, total = carry;
    for (int w = 0; w < JPG_T / 64; ++w) { const uint32_t s = s_wbits[w]; total += s; if (w < wv) off += s; }
    if (act) {
      sink.fill = off & 31; sink.wi = off >> 5;
      jpg_code_block<true>(row, pred, dc_tab, ac_tab, sink);
      sink.flush();
    }
    const bool last = g0 + JPG_GROUP >= g.nb;
    if (last && (total & 7)) {   // the interval ends: 1-bits up to the byte
      if (t == 0) atomicOr(&s_stage[total >> 5], (0xffu >> (total & 7)) << (24 - 8 * ((total >> 3) & 3)));
      total = (total + 7) & ~7u;
    }
    __syncthreads();
    // ---- 3. the whole bytes leave, a zero behind every FF: a run of bytes per thread, the FFs in front of it by a scan
    const uint32_t nbytes = total >> 3;
    const uint32_t per = (((nbytes + JPG_T - 1) / JPG_T) + 3) & ~3u;
    const uint32_t b0 = min((uint32_t)t * per, nbytes), b1 = min(b0 + per, nbytes);
    uint32_t ff = 0;
    for (uint32_t i = b0; i < b1; ++i) ff += ((s_stage[i >> 2] >> (24 - 8 * (i & 3))) & 255u) == 255u;
    const uint32_t ffincl = gs_wave_scan_incl_u32(ff);
    if (lane == 63) s_wff[wv] = ffincl;
    __syncthreads();
    uint32_t ffoff = ffincl - ff, fftotal = 0;
    for (int w = 0; w < JPG_T / 64; ++w) { const uint32_t s = s_wff[w]; fftotal += s; if (w < wv) ffoff += s; }
    if (EMIT) {
      uint8_t* p = dst + nout + b0 + ffoff;
      for (uint32_t i = b0; i < b1; ++i) {
        const uint32_t v = (s_stage[i >> 2] >> (24 - 8 * (i & 3))) & 255u;
        *p++ = (uint8_t)v;
        if (v == 255u) *p++ = 0;
      }
    }
    nout += nbytes + fftotal;
    // ---- 4. the open byte and the predictors go on to the next group
    const uint32_t part = (total & 7) ? (s_stage[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 255u : 0u;
    const int keep = t < 3 ? (int)(int16_t)(s_coef[(cnt - 3 + t) * JPG_CW] & 0xffffu) : 0;   // the last MCU's last Y (or its Y), Cb, Cr
    __syncthreads();
    for (uint32_t i = t; i <= (total >> 5) + 1; i += JPG_T) s_stage[i] = i == 0 ? part << 24 : 0u;
    if (t < 3) s_pred[t] = keep;
    carry = total & 7;
  }
  if (!EMIT && t == 0) meta[(size_t)f * g.mrows + r] = nout;
}

// One workgroup: every interval's position in its file, the files' offsets in `out`.  A thread walks one frame's intervals; the
// file sizes are scanned across the workgroup.
__global__ __launch_bounds__(JPG_T) void k_jpeg_scan(int N, int mrows, const uint32_t* __restrict__ meta, int64_t* __restrict__ rel,
                                                     int64_t* __restrict__ offsets) {
  __shared__ long long s_sz[JPG_T];
  const int t = threadIdx.x;
  long long run = 0;
  for (int f0 = 0; f0 < N; f0 += JPG_T) {
    const int f = f0 + t;
    long long sz = 0;
    if (f < N) {
      long long at = 0;
      for (int r = 0; r < mrows; ++r) {
        const size_t s = (size_t)f * mrows + r;
        rel[s] = at;
        at += (r > 0 ? 2 : 0) + (long long)meta[s];
      }
      sz = JPG_HDR + at + 2;
    }
    s_sz[t] = sz;
    __syncthreads();
    for (int d = 1; d < JPG_T; d <<= 1) {
      const long long v = t >= d ? s_sz[t - d] : 0;
      __syncthreads();
      s_sz[t] += v;
      __syncthreads();
    }
    if (f < N) offsets[f] = run + s_sz[t] - sz;
    run += s_sz[JPG_T - 1];
    __syncthreads();
  }
  if (t == 0) offsets[N] = run;
}

// SOI .. SOS as libjpeg writes them: APP0 JFIF 1.01, two DQT, SOF0, four DHT, DRI, SOS
void jpg_build_header(JpgHeader& h, const JpgLayout& jl, int H, int W, const uint8_t* qtables) {
  uint8_t* p = h.b;
  auto put = [&p](std::initializer_list<int> bytes) { for (int v : bytes) *p++ = (uint8_t)v; };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int tab = 0; tab < 2; ++tab) {
    put({0xFF, 0xDB, 0, 67, tab});
    for (int k = 0; k < 64; ++k) *p++ = qtables[64 * tab + JPG_ZIGZAG[k]];
  }
  put({0xFF, 0xC0, 0, 17, 8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, jl.sub ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int k = 0; k < 4; ++k) {   // DC 0, AC 0, DC 1, AC 1
    const int ac = k & 1, tab = k >> 1, nvals = ac ? 162 : 12;
    put({0xFF, 0xC4, 0, 19 + nvals, (ac << 4) | tab});
    for (int l = 0; l < 16; ++l) *p++ = ac ? JPG_AC_BITS[tab][l] : JPG_DC_BITS[tab][l];
    for (int v = 0; v < nvals; ++v) *p++ = ac ? JPG_AC_VALS[tab][v] : (uint8_t)v;
  }
  put({0xFF, 0xDD, 0, 4, jl.mcols >> 8, jl.mcols & 255});
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
}

}  // namespace

extern "C" {

size_t mi355gs_jpeg_rgb8_scratch_bytes(int N, int H, int W, int subsampling) {
  const JpgLayout jl(N, H, W, subsampling);
  return jl.ok ? jl.total : 0;
}

size_t mi355gs_jpeg_rgb8_stream_bytes(int N, int H, int W, int subsampling) {
  const JpgLayout jl(N, H, W, subsampling);
  return jl.ok ? (size_t)N * jl.file_max : 0;
}

int mi355gs_jpeg_rgb8(void* stream_, int N, int H, int W, int subsampling, const uint8_t* qtables, const uint8_t* frames, void* scratch,
                      uint8_t* out, size_t out_bytes, int64_t* offsets) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const JpgLayout jl(N, H, W, subsampling);
  if (!jl.ok || !qtables || !frames || !scratch || !out || !offsets || ((uintptr_t)scratch & 15) || ((uintptr_t)offsets & 7)) return MI355GS_EINVAL;
  JpgQuant qt;
  for (int i = 0; i < 128; ++i) {
    if (qtables[i] == 0) return MI355GS_EINVAL;
    qt.q[i >> 6][i & 63] = qtables[i];
  }
  JpgHeader hdr;
  memset(&hdr, 0, sizeof(hdr));
  jpg_build_header(hdr, jl, H, W, qtables);
  const JpgGeom g{H, W, jl.sub, jl.bpm, jl.mcols, jl.mrows, jl.nb};
  uint32_t* coef = (uint32_t*)((char*)scratch + jl.coef);
  uint32_t* meta = (uint32_t*)((char*)scratch + jl.meta);
  int64_t* rel = (int64_t*)((char*)scratch + jl.rel);
  GS_KRANGE("jpeg_rows");
  hipLaunchKernelGGL(k_jpeg_rows<false>, dim3(jl.mrows, N), dim3(JPG_T), 0, stream, g, qt, frames, coef, meta, (const int64_t*)rel,
                     (const int64_t*)offsets, out, out_bytes, hdr);
  GS_CHECK_LAUNCH("jpeg_rows");
  GS_KRANGE("jpeg_scan");
  hipLaunchKernelGGL(k_jpeg_scan, dim3(1), dim3(JPG_T), 0, stream, N, jl.mrows, (const uint32_t*)meta, rel, offsets);
  GS_CHECK_LAUNCH("jpeg_scan");
  GS_KRANGE("jpeg_emit");
  hipLaunchKernelGGL(k_jpeg_rows<true>, dim3(jl.mrows + 1, N), dim3(JPG_T), 0, stream, g, qt, frames, coef, meta, (const int64_t*)rel,
                     (const int64_t*)offsets, out, out_bytes, hdr);
  GS_CHECK_LAUNCH("jpeg_emit");
  return MI355GS_OK;
}

}  // extern "C"
