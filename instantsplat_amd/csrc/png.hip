// PNG encoding of 8-bit RGB frames on the device (include/mi355gs.h, mi355gs_png_rgb8): Paeth filter, literal-only deflate with
// an optimal length-limited Huffman code per block, Adler-32, CRC-32 and the chunk framing.  The frames are interleaved
// [N][H][W][3] bytes — exactly a PNG scanline's layout — so nothing is rearranged on the way.
//
// The stream (fixed; tests/png_util.py restates it on the host and predicts every byte count):
//   signature, IHDR, one IDAT per block of `R` filtered rows, one IDAT with the 4 Adler-32 bytes, IEND.
//   A block = one dynamic-Huffman deflate block without matches (HLIT 257, HDIST 1, HCLEN 19; the code-length code is the flat
//   4-bit code, so the header is 74 + 258 x 4 = 1106 bits at a fixed position) followed by an empty stored block, which ends
//   every block on a byte: blocks concatenate bytewise, and every chunk's CRC is local to one workgroup.
//
// Three launches whatever N is:
//   k_png_blocks (blocks, N): filter + histogram, the code (package-merge, all 256 threads), the bits into the block's slot
//   k_png_scan   (1):         chunk positions, file offsets, the Adler-32 of every frame
//   k_png_gather (blocks + 1, N): slots and framing to their final places, the chunks' CRC-32
#include "common.h"
#include <string.h>

namespace {

constexpr int PNG_T = 256;                     // threads of every workgroup here
constexpr int PNG_MAX_BLOCK = 65536;           // filtered bytes of one block
constexpr int PNG_MAX_W = 21845;               // 3 W + 1 <= 65536
constexpr int PNG_K = 16;                      // symbols a thread encodes per round
constexpr int PNG_ROUND = PNG_T * PNG_K;
constexpr int PNG_HDR_BITS = 1106;
constexpr int PNG_LEVELS = 15;                 // deflate's code length limit
// staging of one round: zlib header + block header + 4096 codes of up to 15 bits + the empty stored block
constexpr int PNG_STAGE_WORDS = (16 + PNG_HDR_BITS + PNG_ROUND * PNG_LEVELS + 3 + 7 + 32 + 31) / 32 + 3;
constexpr uint32_t PNG_ADLER = 65521u;
constexpr uint32_t PNG_CRC_POLY = 0xEDB88320u;

// data bytes of a block's IDAT at most: an optimal code costs no more than the flat 9-bit one (257 symbols), so
// sum f l <= 9 (n + 1)
__host__ __device__ inline size_t png_data_bound(size_t nbytes, bool first) {
  return (first ? 2 : 0) + (PNG_HDR_BITS + 9 * (nbytes + 1) + 3 + 7) / 8 + 4;
}

struct PngLayout {
  bool ok = false;
  int R = 0, rb = 0, nblk = 0, last_rows = 0;
  size_t slot = 0;                               // bytes per (frame, block) slot, a multiple of 16
  size_t slots = 0, meta = 0, rel = 0, adler = 0, total = 0;   // offsets into scratch
  size_t file_max = 0;                           // bound on one file
  __host__ PngLayout(int N, int H, int W, int R_) {
    if (N <= 0 || H <= 0 || W <= 0 || R_ < 0 || N > 65535 || W > PNG_MAX_W) return;
    rb = 3 * W + 1;
    R = R_ == 0 ? (PNG_MAX_BLOCK / rb > 0 ? PNG_MAX_BLOCK / rb : 1) : R_;
    if ((long long)R * rb > PNG_MAX_BLOCK) return;
    nblk = (int)(((long long)H + R - 1) / R);
    last_rows = H - (nblk - 1) * R;
    if ((long long)N * nblk > 0x7fffffffLL) return;
    const size_t full = (size_t)(R < H ? R : H) * rb;
    slot = (png_data_bound(full, true) + 4 + 15) & ~(size_t)15;
    const size_t S = (size_t)N * nblk;
    size_t o = 0;
    slots = o; o += gs_align(S * slot);
    meta = o; o += gs_align(S * 4 * sizeof(uint32_t));    // per slot: data bytes, Adler A, Adler B of the block alone, unused
    rel = o; o += gs_align(S * sizeof(int64_t));          // per slot: the chunk's position behind the file's IHDR
    adler = o; o += gs_align((size_t)N * sizeof(uint32_t));
    total = o;
    file_max = 33 + 16 + 12;
    if (nblk == 1) file_max += 12 + png_data_bound((size_t)last_rows * rb, true);
    else file_max += 12 + png_data_bound(full, true) + (size_t)(nblk - 2) * (12 + png_data_bound(full, false)) +
                     12 + png_data_bound((size_t)last_rows * rb, false);
    if (file_max > ((size_t)1 << 62) / (size_t)N) return;
    ok = true;
  }
};

// ---- CRC-32 arithmetic (reflected: bit 31 is x^0), as zlib's crc32_combine does it
__host__ __device__ constexpr uint32_t png_times_x(uint32_t b) { return (b & 1u) ? (b >> 1) ^ PNG_CRC_POLY : b >> 1; }
__device__ inline uint32_t png_gfmul(uint32_t a, uint32_t b) {   // a(x) b(x) mod P
  uint32_t p = 0;
  for (uint32_t m = 0x80000000u; m && a; m >>= 1) {
    if (a & m) { p ^= b; a &= ~m; }
    b = png_times_x(b);
  }
  return p;
}
// x^(8 L) mod P for every span length a chunk of at most 4 + png_data_bound(65536) bytes gives 256 threads
constexpr int PNG_XP8 = 320;
static_assert((4 + 2 + (PNG_HDR_BITS + 9 * (PNG_MAX_BLOCK + 1) + 10) / 8 + 4 + PNG_T - 1) / PNG_T < PNG_XP8, "span table too short");
struct PngXp8 { uint32_t v[PNG_XP8]; };
constexpr PngXp8 png_make_xp8() {
  PngXp8 t{};
  uint32_t b = 0x80000000u;
  for (int i = 0; i < PNG_XP8; ++i) {
    t.v[i] = b;
    for (int k = 0; k < 8; ++k) b = png_times_x(b);
  }
  return t;
}
__device__ const PngXp8 k_png_xp8 = png_make_xp8();

// the 74 fixed bits of a block's header: BFINAL 0, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15, then the 19 code-length-code lengths in
// the format's order (16, 17, 18: 0; the sixteen lengths 0..15: 4)
struct PngHdr { uint32_t w[3]; };
constexpr PngHdr png_make_hdr() {
  PngHdr h{};
  auto put = [&h](int bit, uint32_t v) { h.w[bit >> 5] |= v << (bit & 31); if ((bit & 31) > 29) h.w[(bit >> 5) + 1] |= v >> (32 - (bit & 31)); };
  put(1, 2); put(13, 15);
  for (int k = 0; k < 16; ++k) put(26 + 3 * k, 4);
  return h;
}

__device__ inline void png_stage_or(uint32_t* stage, uint32_t bit, uint32_t v, uint32_t nbits) {   // nbits <= 32, v < 2^nbits
  const uint64_t s = (uint64_t)v << (bit & 31);
  atomicOr(&stage[bit >> 5], (uint32_t)s);
  if ((bit & 31) + nbits > 32) atomicOr(&stage[(bit >> 5) + 1], (uint32_t)(s >> 32));
}

// One workgroup per block of R rows of one frame.  LDS: the block's filtered bytes (64 KiB), the per-wave histograms, the
// package-merge lists with one prefix count per item and level, the code table and one round of output bits.
__global__ __launch_bounds__(PNG_T) void k_png_blocks(int H, int W, int R, const uint8_t* __restrict__ frames, uint8_t* __restrict__ slots,
                                                      size_t slot_bytes, uint32_t* __restrict__ meta) {
  __shared__ alignas(16) uint32_t s_res32[PNG_MAX_BLOCK / 4 + 4];
  __shared__ uint32_t s_hist[PNG_T / 64][256];
  __shared__ uint32_t s_cnt[260], s_w[260], s_len[260], s_cl[260];
  __shared__ uint16_t s_sym[260];
  __shared__ uint32_t s_lst[2][520];
  __shared__ uint16_t s_npk[PNG_LEVELS][520];
  __shared__ uint32_t s_m[16], s_nl[16], s_blc[16], s_next[16], s_wsum[PNG_T / 64];
  __shared__ unsigned long long s_ad[PNG_T / 64][2];
  __shared__ uint32_t s_stage[PNG_STAGE_WORDS];
  uint8_t* s_res = (uint8_t*)s_res32;

  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int blk = blockIdx.x, nblk = gridDim.x, f = blockIdx.y;
  const int rb = 3 * W + 1, row0 = blk * R;
  const int rows = min(R, H - row0), nb = rows * rb;
  const uint8_t* img = frames + (size_t)f * (size_t)H * (size_t)W * 3;

  for (int i = t; i < (PNG_T / 64) * 256; i += PNG_T) (&s_hist[0][0])[i] = 0;
  for (int i = t; i < PNG_STAGE_WORDS; i += PNG_T) s_stage[i] = 0;
  if (t < 16) s_blc[t] = 0;
  __syncthreads();

  // ---- 1. Paeth residuals (filter byte 4 in front of every row) into LDS, the histogram, the Adler sums.  The predictor reads
  // the raw row above from the frame, so the block depends on no other block.  Byte loads: any base address will do.
  unsigned long long sum_d = 0, sum_w = 0;
  for (int r = 0; r < rows; ++r) {
    const int y = row0 + r;
    const uint8_t* cur = img + (size_t)y * 3 * W;
    const uint8_t* up = cur - (ptrdiff_t)3 * W;   // read only where y > 0
    for (int c0 = 0; c0 < rb; c0 += PNG_T) {
      const int c = c0 + t;
      const bool act = c < rb;
      uint32_t v = 1;
      if (act) {
        if (c == 0) v = 4;
        else {
          const int x = c - 1;
          const int a = x >= 3 ? cur[x - 3] : 0, b = y > 0 ? up[x] : 0, cc = (x >= 3 && y > 0) ? up[x - 3] : 0;
          const int pa = abs(b - cc), pb = abs(a - cc), pc = abs(a + b - 2 * cc);
          const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : cc);
          v = (uint32_t)(cur[x] - pred) & 255u;
        }
        const int idx = r * rb + c;
        s_res[idx] = (uint8_t)v;
        sum_d += v;
        sum_w += (unsigned long long)(nb - idx) * v;
      }
      // residual 0 is the hot bin: one add of the wave's count of zeros instead of up to 64 atomics on one address
      const unsigned long long zeros = __ballot(act && v == 0);
      if (act && v != 0) atomicAdd(&s_hist[wv][v], 1u);
      if (lane == 0 && zeros) s_hist[wv][0] += (uint32_t)__popcll(zeros);   // no other lane of the wave touches bin 0
    }
  }
  sum_d = gs_wave_sum_row3(sum_d);
  sum_w = gs_wave_sum_row3(sum_w);
  if (lane == 63) { s_ad[wv][0] = sum_d; s_ad[wv][1] = sum_w; }
  __syncthreads();
  {
    uint32_t c = 0;
    for (int w = 0; w < PNG_T / 64; ++w) c += s_hist[w][t];
    s_cnt[t] = c;
    s_len[t] = 0;
    if (t == 0) { s_cnt[256] = 1; s_len[256] = 0; }   // end of block
  }
  __syncthreads();

  // ---- 2. the code: minimum sum f l under l <= 15 by package-merge in its prefix-count form.
  // Sort the used symbols by (count, symbol): every symbol counts the symbols in front of it.
  int n = 0;
  for (int s = t; s < 257; s += PNG_T) {
    const uint32_t c = s_cnt[s];
    int rank = 0, used = 0;
    for (int u = 0; u < 257; ++u) {
      const uint32_t cu = s_cnt[u];
      used += cu != 0;
      rank += cu != 0 && (cu < c || (cu == c && u < s));
    }
    n = used;
    if (c != 0) { s_w[rank] = c; s_sym[rank] = (uint16_t)s; }
  }
  __syncthreads();
  // Level 1 is the leaves; level k merges the leaves with the pairwise sums of level k - 1 (ties: the leaf first).  Per item only
  // the number of packages in front of it is kept.
  for (int i = t; i < n; i += PNG_T) { s_lst[0][i] = s_w[i]; s_npk[0][i] = 0; }
  if (t == 0) s_m[0] = 0;
  int prev_len = n, pbuf = 0;
  for (int lv = 1; lv < PNG_LEVELS; ++lv) {
    __syncthreads();
    const uint32_t* prev = s_lst[pbuf];
    uint32_t* cur = s_lst[pbuf ^ 1];
    const int m = prev_len >> 1;
    for (int i = t; i < n; i += PNG_T) {
      const uint32_t w = s_w[i];
      int lo = 0, hi = m;   // packages lighter than the leaf
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (prev[2 * mid] + prev[2 * mid + 1] < w) lo = mid + 1; else hi = mid; }
      cur[i + lo] = w; s_npk[lv][i + lo] = (uint16_t)lo;
    }
    for (int j = t; j < m; j += PNG_T) {
      const uint32_t pw = prev[2 * j] + prev[2 * j + 1];
      int lo = 0, hi = n;   // leaves no heavier than the package
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (s_w[mid] <= pw) lo = mid + 1; else hi = mid; }
      cur[j + lo] = pw; s_npk[lv][j + lo] = (uint16_t)j;
    }
    if (t == 0) s_m[lv] = (uint32_t)m;
    prev_len = n + m; pbuf ^= 1;
  }
  __syncthreads();
  if (t == 0) {   // walk back: of a level's first `take` items p are packages; the other take - p are the lightest leaves
    int take = 2 * n - 2;
    for (int lv = PNG_LEVELS - 1; lv >= 0; --lv) {
      const int m = (int)s_m[lv], len = n + m;
      if (take > len) take = len;
      const int p = take < len ? (int)s_npk[lv][take] : m;
      s_nl[lv] = (uint32_t)(take - p);
      take = 2 * p;
    }
  }
  __syncthreads();
  for (int i = t; i < n; i += PNG_T) {
    uint32_t l = 0;
    for (int lv = 0; lv < PNG_LEVELS; ++lv) l += s_nl[lv] > (uint32_t)i;
    if (n == 1) l = 1;
    s_len[s_sym[i]] = l;
    atomicAdd(&s_blc[l], 1u);
  }
  __syncthreads();
  if (t == 0) {   // canonical codes: the first code of every length
    uint32_t code = 0;
    s_next[0] = 0;
    for (int l = 1; l <= PNG_LEVELS; ++l) { code = (code + (l > 1 ? s_blc[l - 1] : 0)) << 1; s_next[l] = code; }
  }
  __syncthreads();
  const uint32_t hdr0 = blk == 0 ? 16u : 0u;   // the zlib header 78 01 opens the first block's chunk
  for (int s = t; s < 258; s += PNG_T) {
    uint32_t l = 1;   // 257: the one distance code
    if (s < 257) {
      l = s_len[s];
      uint32_t code = s_next[l], rev = 0;
      for (int u = 0; u < s; ++u) code += s_len[u] == l;
      for (uint32_t k = 0; k < l; ++k) rev |= ((code >> k) & 1u) << (l - 1 - k);   // Huffman codes go out most significant bit first
      s_cl[s] = l ? (rev | (l << 16)) : 0;
    }
    const uint32_t rev4 = ((l & 1) << 3) | ((l & 2) << 1) | ((l & 4) >> 1) | ((l & 8) >> 3);
    png_stage_or(s_stage, hdr0 + 74 + 4 * (uint32_t)s, rev4, 4);
  }
  if (t == 0) {
    constexpr PngHdr h = png_make_hdr();
    if (blk == 0) atomicOr(&s_stage[0], 0x0178u);
    png_stage_or(s_stage, hdr0, h.w[0], 32);
    png_stage_or(s_stage, hdr0 + 32, h.w[1], 32);
    png_stage_or(s_stage, hdr0 + 64, h.w[2], 10);
  }

  // ---- 3. the bits, in rounds of 16 symbols per thread: lengths, a workgroup scan, then every thread assembles whole words in
  // a register and ORs them into the round's staging words in LDS; whole words leave for the slot, the partial one is carried.
  uint32_t* slot32 = (uint32_t*)(slots + ((size_t)f * nblk + blk) * slot_bytes);
  const size_t slot_words = slot_bytes / 4;
  const int nsym = nb + 1;
  uint32_t carry = hdr0 + PNG_HDR_BITS, total = 0, data_bytes = 0;
  size_t wout = 0;
  for (int base = 0; base < nsym; base += PNG_ROUND) {
    __syncthreads();
    const int i0 = base + t * PNG_K;
    const int cnt = min(max(nsym - i0, 0), PNG_K);
    uint32_t q[4] = {0, 0, 0, 0};
    if (cnt > 0) { const uint4 v = ((const uint4*)s_res32)[i0 >> 4]; q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w; }
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < PNG_K; ++k)
      if (k < cnt) bits += s_cl[i0 + k == nb ? 256u : (q[k >> 2] >> (8 * (k & 3))) & 255u] >> 16;
    const uint32_t incl = gs_wave_scan_incl_u32(bits);
    if (lane == 63) s_wsum[wv] = incl;
    __syncthreads();
    uint32_t off = carry + incl - bits;
    total = carry;
    for (int w = 0; w < PNG_T / 64; ++w) { const uint32_t s = s_wsum[w]; total += s; if (w < wv) off += s; }
    uint64_t acc = 0;
    uint32_t fill = off & 31, wi = off >> 5;
#pragma unroll
    for (int k = 0; k < PNG_K; ++k)
      if (k < cnt) {
        const uint32_t cl = s_cl[i0 + k == nb ? 256u : (q[k >> 2] >> (8 * (k & 3))) & 255u];
        acc |= (uint64_t)(cl & 0xffffu) << fill;
        fill += cl >> 16;
        if (fill >= 32) { atomicOr(&s_stage[wi++], (uint32_t)acc); acc >>= 32; fill -= 32; }
      }
    if (acc) atomicOr(&s_stage[wi], (uint32_t)acc);
    const bool last = base + PNG_ROUND >= nsym;
    if (last) {   // the empty stored block: 3 header bits (BFINAL in the frame's last block), padding, LEN 0000, NLEN FFFF
      if (t == 0) {
        if (blk == nblk - 1) png_stage_or(s_stage, total, 1, 3);
        png_stage_or(s_stage, ((total + 3 + 7) & ~7u) + 16, 0xffffu, 16);
      }
      total = ((total + 3 + 7) & ~7u) + 32;
    }
    __syncthreads();
    const uint32_t nw = last ? (total + 31) >> 5 : total >> 5;
    for (uint32_t i = t; i < nw && wout + i < slot_words; i += PNG_T) slot32[wout + i] = s_stage[i];   // (an optimal code never reaches the slot's end)
    const uint32_t part = s_stage[nw];
    __syncthreads();
    for (uint32_t i = t; i <= nw; i += PNG_T) s_stage[i] = 0;
    if (t == 0) s_stage[0] = part;
    if (last) data_bytes = (uint32_t)(4 * wout) + (total >> 3);   // (total is a multiple of 8 now)
    wout += nw; carry = total & 31;
  }
  if (t == 0) {
    unsigned long long d = 0, w = 0;
    for (int k = 0; k < PNG_T / 64; ++k) { d += s_ad[k][0]; w += s_ad[k][1]; }
    uint32_t* m = meta + ((size_t)f * nblk + blk) * 4;
    m[0] = min(data_bytes, (uint32_t)slot_bytes - 4u);        // data bytes
    m[1] = (uint32_t)((1 + d) % PNG_ADLER);                  // Adler-32 of the block's bytes alone
    m[2] = (uint32_t)(((unsigned long long)nb + w) % PNG_ADLER);
    m[3] = 0;
  }
}

// One workgroup: every chunk's position in its file, the files' offsets in `out`, every frame's Adler-32 (the blocks' partial
// sums combined in block order).  A thread walks one frame's blocks; the file sizes are scanned across the workgroup.
__global__ __launch_bounds__(PNG_T) void k_png_scan(int N, int nblk, int H, int R, int rb, const uint32_t* __restrict__ meta,
                                                    int64_t* __restrict__ rel, uint32_t* __restrict__ adler, int64_t* __restrict__ offsets) {
  __shared__ long long s_sz[PNG_T];
  const int t = threadIdx.x;
  long long run = 0;
  for (int f0 = 0; f0 < N; f0 += PNG_T) {
    const int f = f0 + t;
    long long sz = 0;
    if (f < N) {
      unsigned long long A = 1, B = 0;
      long long at = 0;
      for (int b = 0; b < nblk; ++b) {
        const size_t s = (size_t)f * nblk + b;
        const uint32_t* m = meta + s * 4;
        rel[s] = at;
        at += 12 + (long long)m[0];
        const unsigned long long n2 = (unsigned long long)min(R, H - b * R) * rb;
        B = (B + m[2] + (n2 % PNG_ADLER) * ((A + PNG_ADLER - 1) % PNG_ADLER)) % PNG_ADLER;
        A = (A + m[1] + PNG_ADLER - 1) % PNG_ADLER;
      }
      adler[f] = (uint32_t)((B << 16) | A);
      sz = 33 + at + 16 + 12;
    }
    s_sz[t] = sz;
    __syncthreads();
    for (int d = 1; d < PNG_T; d <<= 1) {
      const long long v = t >= d ? s_sz[t - d] : 0;
      __syncthreads();
      s_sz[t] += v;
      __syncthreads();
    }
    if (f < N) offsets[f] = run + s_sz[t] - sz;
    run += s_sz[PNG_T - 1];
    __syncthreads();
  }
  if (t == 0) offsets[N] = run;
}

struct PngFraming { uint8_t head[33]; uint8_t iend[12]; };   // signature + IHDR and IEND, built by the host per call

__device__ inline uint32_t png_crc_byte(const uint32_t* tab, uint32_t crc, uint32_t byte) { return tab[(crc ^ byte) & 255u] ^ (crc >> 8); }

// Workgroup (b, f): block b's slot becomes the chunk length | IDAT | data | CRC at its place in file f; workgroup (blocks, f)
// writes the signature, IHDR, the Adler-32 chunk and IEND.  CRC: every thread takes one span of the chunk with zero init — the
// spans are equally long and right-aligned, so the short one is the first and carries the 0xFFFFFFFF init — and a tree of
// multiplications by x^(8 span), x^(16 span), ... mod P combines them.
__global__ __launch_bounds__(PNG_T) void k_png_gather(int nblk, const uint8_t* __restrict__ slots, size_t slot_bytes,
                                                      const uint32_t* __restrict__ meta, const int64_t* __restrict__ rel,
                                                      const uint32_t* __restrict__ adler, const int64_t* __restrict__ offsets,
                                                      uint8_t* __restrict__ out, PngFraming fr) {
  __shared__ uint32_t s_tab[256], s_crc[PNG_T];
  const int t = threadIdx.x, b = blockIdx.x, f = blockIdx.y;
  {
    uint32_t c = (uint32_t)t;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? PNG_CRC_POLY ^ (c >> 1) : c >> 1;
    s_tab[t] = c;
  }
  __syncthreads();
  uint8_t* file = out + offsets[f];
  if (b == nblk) {
    if (t < 33) file[t] = fr.head[t];
    uint8_t* tail = out + offsets[f + 1] - 28;
    if (t == 64) {
      const uint32_t a = adler[f];
      uint32_t crc = 0xffffffffu;
      const uint32_t by[8] = {'I', 'D', 'A', 'T', a >> 24, (a >> 16) & 255u, (a >> 8) & 255u, a & 255u};
      tail[0] = 0; tail[1] = 0; tail[2] = 0; tail[3] = 4;
#pragma unroll
      for (int k = 0; k < 8; ++k) { tail[4 + k] = (uint8_t)by[k]; crc = png_crc_byte(s_tab, crc, by[k]); }
      crc = ~crc;
      tail[12] = (uint8_t)(crc >> 24); tail[13] = (uint8_t)(crc >> 16); tail[14] = (uint8_t)(crc >> 8); tail[15] = (uint8_t)crc;
    }
    if (t >= 128 && t < 140) tail[16 + t - 128] = fr.iend[t - 128];
    return;
  }
  const size_t slot = (size_t)f * nblk + b;
  const uint32_t len = meta[slot * 4];
  const uint8_t* src = slots + slot * slot_bytes;   // 16-byte aligned
  uint8_t* dst = file + 33 + rel[slot];
  if (t < 4) dst[t] = (uint8_t)(len >> (24 - 8 * t));
  else if (t < 8) dst[t] = (uint8_t)"IDAT"[t - 4];
  // the data: byte stores up to the destination's first word boundary and behind its last, word stores between, every word
  // funnelled from two aligned words of the slot
  uint8_t* d = dst + 8;
  const uint32_t head = min(len, (uint32_t)((4 - ((uintptr_t)d & 3)) & 3));
  const uint32_t nwords = (len - head) >> 2;
  if ((uint32_t)t < head) d[t] = src[t];
  {
    const uint32_t* s32 = (const uint32_t*)src;
    uint32_t* d32 = (uint32_t*)(d + head);
    const uint32_t sh = 8 * head;
    for (uint32_t j = t; j < nwords; j += PNG_T) {
      const uint32_t lo = s32[j];
      d32[j] = sh ? (lo >> sh) | (s32[j + 1] << (32 - sh)) : lo;   // the slot has 4 bytes of room behind its longest data
    }
  }
  for (uint32_t i = head + 4 * nwords + t; i < len; i += PNG_T) d[i] = src[i];
  // the chunk's CRC-32 over type + data
  const int total = (int)len + 4, L = (total + PNG_T - 1) / PNG_T;
  const int hi = total - (PNG_T - 1 - t) * L, lo = max(hi - L, 0);
  uint32_t crc = (hi > 0 && lo == 0) ? 0xffffffffu : 0u;
  for (int i = lo; i < hi; ++i) crc = png_crc_byte(s_tab, crc, i < 4 ? (uint32_t)"IDAT"[i] : (uint32_t)src[i - 4]);
  s_crc[t] = crc;
  uint32_t c = k_png_xp8.v[min(L, PNG_XP8 - 1)];   // L < PNG_XP8 for every block the entry point accepts
  for (int s = 1; s < PNG_T; s <<= 1) {
    __syncthreads();
    if ((t & (2 * s - 1)) == 2 * s - 1) s_crc[t] = png_gfmul(s_crc[t - s], c) ^ s_crc[t];
    c = png_gfmul(c, c);
  }
  if (t == PNG_T - 1) {
    crc = ~s_crc[t];
    uint8_t* e = d + len;
    e[0] = (uint8_t)(crc >> 24); e[1] = (uint8_t)(crc >> 16); e[2] = (uint8_t)(crc >> 8); e[3] = (uint8_t)crc;
  }
}

uint32_t png_host_crc(const uint8_t* p, int n) {
  uint32_t crc = 0xffffffffu;
  for (int i = 0; i < n; ++i) {
    crc ^= p[i];
    for (int k = 0; k < 8; ++k) crc = (crc & 1u) ? PNG_CRC_POLY ^ (crc >> 1) : crc >> 1;
  }
  return ~crc;
}
void png_put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

}  // namespace

extern "C" {

size_t mi355gs_png_rgb8_scratch_bytes(int N, int H, int W, int rows_per_block) {
  const PngLayout pl(N, H, W, rows_per_block);
  return pl.ok ? pl.total : 0;
}

size_t mi355gs_png_rgb8_stream_bytes(int N, int H, int W, int rows_per_block) {
  const PngLayout pl(N, H, W, rows_per_block);
  return pl.ok ? (size_t)N * pl.file_max : 0;
}

int mi355gs_png_rgb8(void* stream_, int N, int H, int W, int rows_per_block, const uint8_t* frames, void* scratch, uint8_t* out,
                     int64_t* offsets) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const PngLayout pl(N, H, W, rows_per_block);
  if (!pl.ok || !frames || !scratch || !out || !offsets || ((uintptr_t)scratch & 15) || ((uintptr_t)offsets & 7)) return MI355GS_EINVAL;
  uint8_t* slots = (uint8_t*)scratch + pl.slots;
  uint32_t* meta = (uint32_t*)((char*)scratch + pl.meta);
  int64_t* rel = (int64_t*)((char*)scratch + pl.rel);
  uint32_t* adler = (uint32_t*)((char*)scratch + pl.adler);
  PngFraming fr;
  const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
  memcpy(fr.head, sig, 8);
  png_put_be32(fr.head + 8, 13);
  memcpy(fr.head + 12, "IHDR", 4);
  png_put_be32(fr.head + 16, (uint32_t)W);
  png_put_be32(fr.head + 20, (uint32_t)H);
  fr.head[24] = 8; fr.head[25] = 2; fr.head[26] = 0; fr.head[27] = 0; fr.head[28] = 0;   // depth 8, colour type 2 (RGB)
  png_put_be32(fr.head + 29, png_host_crc(fr.head + 12, 17));
  png_put_be32(fr.iend, 0);
  memcpy(fr.iend + 4, "IEND", 4);
  png_put_be32(fr.iend + 8, png_host_crc(fr.iend + 4, 4));
  GS_KRANGE("png_blocks");
  hipLaunchKernelGGL(k_png_blocks, dim3(pl.nblk, N), dim3(PNG_T), 0, stream, H, W, pl.R, frames, slots, pl.slot, meta);
  GS_CHECK_LAUNCH("png_blocks");
  GS_KRANGE("png_scan");
  hipLaunchKernelGGL(k_png_scan, dim3(1), dim3(PNG_T), 0, stream, N, pl.nblk, H, pl.R, pl.rb, (const uint32_t*)meta, rel, adler, offsets);
  GS_CHECK_LAUNCH("png_scan");
  GS_KRANGE("png_gather");
  hipLaunchKernelGGL(k_png_gather, dim3(pl.nblk + 1, N), dim3(PNG_T), 0, stream, pl.nblk, (const uint8_t*)slots, pl.slot,
                     (const uint32_t*)meta, (const int64_t*)rel, (const uint32_t*)adler, (const int64_t*)offsets, out, fr);
  GS_CHECK_LAUNCH("png_gather");
  return MI355GS_OK;
}

}  // extern "C"
