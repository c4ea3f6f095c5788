// MASt3R's transformer trunk on the device (include/mi355gs.h, mi355gs_vit_encode / mi355gs_vit_decode): the ViT encoder,
// decoder_embed and the two cross-attending decoders of dust3r/model.py:127-190, float32 throughout.
//
// Activations are [token][channel] float32 matrices in the caller's scratch; a linear layer is  out = epi(A W + bias)  with the
// weights packed [K][N] (torch's weight transposed, once, by the wrapper).
//
//   k_vit_patches    planar images -> [token][3 * 16 * 16] rows (k = (c * 16 + py) * 16 + px, the flattened convolution weight)
//   k_vit_gemm       (mm_tile.h, shared with dpt.hip) 128 rows x (64 or 128) outputs per workgroup, K in chunks of 32 through LDS, v_mfma_f32_32x32x2_f32 (exact
//                    float32: a k-ordered fmaf chain), epilogue: bias; bias + exact-erf GELU; resid + bias.  Rows past M are never
//                    loaded or stored.
//   k_vit_layernorm  a wave per token, the row held in registers: mean, then the sum of squared deviations, fixed lane order.
//   k_vit_attention  64 query rows of one head of one sequence per workgroup; keys in chunks of 64; RoPE2D applied while q and k
//                    are staged; scores and P V through the matrix helper; online softmax (running maximum subtracted, tail
//                    keys masked to -inf before the maximum).  Self- and cross-attention differ only in pointers and strides.
//   k_vit_gather     hook 0 of the decoder: the encoder rows of an edge's image.
// No atomics, no memset, no allocation, no host synchronisation of its own (decode's copy of the host edge list may wait for the
// stream, as the runtime decides for pageable memory); equal bits run to run, and a token's result does not depend on
// which tile it falls in (every row of a tile is an independent chain).
#include "common.h"
#include "mm_tile.h"
#include <math.h>

namespace {

constexpr int VT_T = 256;            // threads of every kernel here (the GEMM's own: mm_tile.h)
constexpr int VT_HD = 64;            // head dimension
constexpr int VT_AQ = 64;            // query rows of an attention workgroup
constexpr int VT_AK = 64;            // keys of a chunk
constexpr int VT_ALD = 65;           // LDS row of the attention tiles: consecutive rows one bank apart
constexpr int VT_MAX_D = 1024;       // widest LayerNorm row a wave holds: 16 values per lane
constexpr int VT_MAX_TOKENS = 4096;
constexpr int VT_PATCH = 16;
constexpr int VT_PATCH_K = 3 * VT_PATCH * VT_PATCH;
constexpr float VT_LN_EPS = 1e-6f;

__device__ __forceinline__ float vt_wave_sum(float v) {   // butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// ---------------------------------------------------------------------------------------------------- patches, gather
// images [V][3][H][W] -> rows [V * Ht * Wt][768]; one float4 (four px of one py) per thread
__global__ __launch_bounds__(VT_T) void k_vit_patches(long long total4, int Ht, int Wt, const float* __restrict__ img, float* __restrict__ rows) {
  const long long e = (long long)blockIdx.x * VT_T + threadIdx.x;
  if (e >= total4) return;
  const int k4 = (int)(e % (VT_PATCH_K / 4));
  const long long tok = e / (VT_PATCH_K / 4);
  const int N = Ht * Wt, W = Wt * VT_PATCH, H = Ht * VT_PATCH;
  const int n = (int)(tok % N);
  const long long v = tok / N;
  const int ty = n / Wt, tx = n - ty * Wt;
  const int k = 4 * k4, c = k / (VT_PATCH * VT_PATCH), py = (k / VT_PATCH) % VT_PATCH, px = k % VT_PATCH;
  const float* src = img + (((size_t)v * 3 + c) * H + (size_t)ty * VT_PATCH + py) * W + (size_t)tx * VT_PATCH + px;
  *(lp_f4*)(rows + (size_t)tok * VT_PATCH_K + k) = *(const lp_f4*)src;
}

// out[e][n][:] = feat[edges[2 e + side]][n][:], one float4 per thread
__global__ __launch_bounds__(VT_T) void k_vit_gather(long long total4, int ND4, int side, const int32_t* __restrict__ edges,
                                                    const lp_f4* __restrict__ feat, lp_f4* __restrict__ out) {
  const long long e = (long long)blockIdx.x * VT_T + threadIdx.x;
  if (e >= total4) return;
  const long long edge = e / ND4;
  const int r = (int)(e - edge * ND4);
  out[e] = feat[(size_t)edges[2 * edge + side] * ND4 + r];
}


// ---------------------------------------------------------------------------------------------------- LayerNorm
// grid (ceil(M / 4)): a wave per row of D <= 1024 values (D a multiple of 64).  in may be out.
__global__ __launch_bounds__(VT_T) void k_vit_layernorm(int M, int D, const float* in, const float* __restrict__ w,
                                                        const float* __restrict__ b, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * (VT_T / 64) + wave;
  if (row >= M) return;   // the whole wave
  const float* src = in + (size_t)row * D;
  float v[VT_MAX_D / 64];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < VT_MAX_D / 64; ++j) {
    v[j] = lane + 64 * j < D ? src[lane + 64 * j] : 0.f;
    s += v[j];
  }
  const float mean = vt_wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < VT_MAX_D / 64; ++j) {
    const float d = lane + 64 * j < D ? v[j] - mean : 0.f;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(vt_wave_sum(q) / (float)D + VT_LN_EPS);
  float* dst = out + (size_t)row * D;
#pragma unroll
  for (int j = 0; j < VT_MAX_D / 64; ++j)
    if (lane + 64 * j < D) dst[lane + 64 * j] = fmaf((v[j] - mean) * rstd, w[lane + 64 * j], b[lane + 64 * j]);
}

// ---------------------------------------------------------------------------------------------------- attention
// RoPE2D of channel d of a head, the channel being the LANE (d = lane): channel d < 32 turns by the token's y, d >= 32 by its x;
// inside a half of 32, channel j pairs with j +- 16 — the value 16 lanes away — and both use frequency j mod 16.
// rope: cos [P][16] then sin [P][16] (float32 cos / sin of float32 angles).  Every lane of the wave calls it (the shuffle); a lane
// whose token does not exist passes t = 0, in = false and receives 0 without touching the table.
__device__ __forceinline__ float vt_rope(float t, bool in, int d, int ty, int tx, const float* __restrict__ rope, int P) {
  const int j = d & 31, p = d < 32 ? ty : tx;
  const float partner = __shfl_xor(t, 16);
  if (!in) return 0.f;
  const float c = rope[p * 16 + (j & 15)], s = rope[(P + p) * 16 + (j & 15)];
  return fmaf(t, c, (j < 16 ? -partner : partner) * s);
}
// the grid position of a token `step` tokens further on (one integer division per thread and kernel, not one per element)
__device__ __forceinline__ void vt_advance(int& ty, int& tx, int step, int Wt) {
  tx += step;
  while (tx >= Wt) { tx -= Wt; ++ty; }
}

// grid (ceil(Nq / 64), heads, sequences), 4 waves.  Sequence s reads q rows [s Nq, (s + 1) Nq) of `q` (row stride ldq floats,
// this head's 64 channels at column 64 head), k / v rows [s Nk, (s + 1) Nk) likewise, and writes out rows [s Nq, ...) (stride ldo).
// A token's grid position is (n / Wt, n % Wt) of its index n inside its sequence, for queries and keys alike.
// Wave w owns rows 32 (w & 1) and, of a 64-wide product, columns 32 (w >> 1): the scores of a chunk first, then its share of O.
__global__ __launch_bounds__(VT_T) void k_vit_attention(int Nq, int Nk, int Wt, int P, const float* __restrict__ q, int ldq,
                                                        const float* __restrict__ k, int ldk, const float* __restrict__ v, int ldv,
                                                        float* __restrict__ out, int ldo, const float* __restrict__ rope) {
  __shared__ float Qs[VT_AQ * VT_ALD];    // [query][d], turned
  __shared__ float Ks[VT_AK * VT_ALD];    // [d][key] of the chunk, turned; then the chunk's scores / probabilities [query][key]
  __shared__ float Vs[VT_AK * VT_ALD];    // [key][d]
  __shared__ float s_alpha[VT_AQ], s_l[VT_AQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rb = wave & 1, cb = wave >> 1;
  const int q0 = blockIdx.x * VT_AQ, head = blockIdx.y, seq = blockIdx.z;
  const float* qb = q + (size_t)seq * Nq * ldq + head * VT_HD;
  const float* kb = k + (size_t)seq * Nk * ldk + head * VT_HD;
  const float* vb = v + (size_t)seq * Nk * ldv + head * VT_HD;

  // staging: this thread's channel is its lane, its rows are wave, wave + 4, ...; the rows' grid positions are carried along
  {
    int ty = (q0 + wave) / Wt, tx = (q0 + wave) - ty * Wt;
    for (int row = wave; row < VT_AQ; row += VT_T / 64) {
      const int n = q0 + row;
      const bool in = n < Nq;
      Qs[row * VT_ALD + lane] = vt_rope(in ? qb[(size_t)n * ldq + lane] : 0.f, in, lane, ty, tx, rope, P);
      vt_advance(ty, tx, VT_T / 64, Wt);
    }
  }
  int kty = wave / Wt, ktx = wave - kty * Wt;   // of key c0 + wave + 4 i: advanced through every chunk in turn
  lp_acc16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  // softmax state of row tid >> 2, kept (equal) by the four threads that share the row
  const int srow = tid >> 2, spart = tid & 3;
  float m_run = -INFINITY, l_run = 0.f;

  for (int c0 = 0; c0 < Nk; c0 += VT_AK) {
    __syncthreads();   // the previous chunk's P and V have been consumed (first round: nothing pending)
    for (int key = wave; key < VT_AK; key += VT_T / 64) {
      const int n = c0 + key;
      const bool in = n < Nk;
      Ks[lane * VT_ALD + key] = vt_rope(in ? kb[(size_t)n * ldk + lane] : 0.f, in, lane, kty, ktx, rope, P);
      Vs[key * VT_ALD + lane] = in ? vb[(size_t)n * ldv + lane] : 0.f;
      vt_advance(kty, ktx, VT_T / 64, Wt);
    }
    __syncthreads();
    lp_acc16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll 4
    for (int kk = 0; kk < VT_HD / 2; ++kk)
      lp_mfma_32x32x2(s, Qs + 32 * rb * VT_ALD + 2 * kk, VT_ALD, Ks + 2 * kk * VT_ALD + 32 * cb, VT_ALD, lane);
    __syncthreads();   // every wave has read the keys: their tile now takes the scores
    {
      const int col = 32 * cb + (lane & 31);
      const bool in = c0 + col < Nk;
#pragma unroll
      for (int r = 0; r < 16; ++r) Ks[(32 * rb + lp_acc_row(r, lane)) * VT_ALD + col] = in ? s[r] * 0.125f : -INFINITY;   // 1 / sqrt(64)
    }
    __syncthreads();
    {
      float* sr = Ks + srow * VT_ALD + 16 * spart;
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) mx = fmaxf(mx, sr[i]);
      mx = fmaxf(mx, __shfl_xor(mx, 1));
      mx = fmaxf(mx, __shfl_xor(mx, 2));
      const float m_new = fmaxf(m_run, mx);        // finite: key c0 of the chunk exists
      const float alpha = expf(m_run - m_new);     // first chunk: exp(-inf) = 0
      float ps = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = expf(sr[i] - m_new);       // masked keys: exp(-inf) = 0
        sr[i] = p;
        ps += p;
      }
      ps += __shfl_xor(ps, 1);
      ps += __shfl_xor(ps, 2);
      l_run = fmaf(l_run, alpha, ps);
      m_run = m_new;
      if (spart == 0) s_alpha[srow] = alpha;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] *= s_alpha[32 * rb + lp_acc_row(r, lane)];
#pragma unroll 4
    for (int kk = 0; kk < VT_AK / 2; ++kk)
      lp_mfma_32x32x2(o, Ks + 32 * rb * VT_ALD + 2 * kk, VT_ALD, Vs + 2 * kk * VT_ALD + 32 * cb, VT_ALD, lane);
  }
  if (spart == 0) s_l[srow] = l_run;
  __syncthreads();
  float* ob = out + (size_t)seq * Nq * ldo + head * VT_HD + 32 * cb + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = 32 * rb + lp_acc_row(r, lane);
    if (q0 + row < Nq) ob[(size_t)(q0 + row) * ldo] = o[r] / s_l[row];
  }
}

// ---------------------------------------------------------------------------------------------------- host side
struct VtPlan {
  bool ok = false;
  int De, Le, He, Dd, Ld, Hd, N;
  int hooks[4];
  VtPlan(const mi355gs_vit_config* c, int Ht, int Wt) {
    if (!c || Ht <= 0 || Wt <= 0 || (long long)Ht * Wt > VT_MAX_TOKENS) return;
    De = c->enc_dim; Le = c->enc_depth; He = c->enc_heads; Dd = c->dec_dim; Ld = c->dec_depth; Hd = c->dec_heads;
    if (De < 64 || De > VT_MAX_D || De % 64 || Dd < 64 || Dd > VT_MAX_D || Dd % 64) return;
    if (He * VT_HD != De || Hd * VT_HD != Dd || Le < 1 || Le > 256 || Ld < 1 || Ld > 256 || c->patch != VT_PATCH) return;
    for (int i = 0; i < 4; ++i) hooks[i] = c->hooks[i];
    if (hooks[0] != 0 || hooks[1] < 1 || hooks[1] >= hooks[2] || hooks[2] >= hooks[3] || hooks[3] != Ld) return;
    N = Ht * Wt;
    ok = true;
  }
  // the blob (include/mi355gs.h), in floats
  static size_t lin(int K, int N_) { return (size_t)K * N_ + N_; }
  size_t enc_block() const { return 2 * (size_t)De + lin(De, 3 * De) + lin(De, De) + 2 * (size_t)De + lin(De, 4 * De) + lin(4 * De, De); }
  size_t dec_block() const { return 8 * (size_t)Dd + lin(Dd, 3 * Dd) + 5 * lin(Dd, Dd) + lin(Dd, 4 * Dd) + lin(4 * Dd, Dd); }
  size_t enc_floats() const { return lin(VT_PATCH_K, De) + Le * enc_block() + 2 * (size_t)De; }
  size_t dec_offset() const { return enc_floats(); }   // decoder_embed, side 1's blocks, side 2's blocks, dec_norm
};

struct VtEncScratch {
  size_t t, qkv, hid, total;
  VtEncScratch(const VtPlan& p, size_t M) {
    size_t o = 0;
    t = o; o += gs_align(M * p.De * 4);
    qkv = o; o += gs_align(M * 3 * p.De * 4);
    hid = o; o += gs_align(M * (size_t)std::max(4 * p.De, VT_PATCH_K) * 4);
    total = o;
  }
};
struct VtDecScratch {
  size_t edges, x[2][2], t, yn, qkv, hid, total;
  VtDecScratch(const VtPlan& p, size_t E) {
    const size_t M = E * p.N;
    size_t o = 0;
    edges = o; o += gs_align(E * 2 * 4);
    for (int s = 0; s < 2; ++s)
      for (int b = 0; b < 2; ++b) { x[s][b] = o; o += gs_align(M * p.Dd * 4); }
    t = o; o += gs_align(M * p.Dd * 4);
    yn = o; o += gs_align(M * p.Dd * 4);
    qkv = o; o += gs_align(M * 3 * p.Dd * 4);
    hid = o; o += gs_align(M * 4 * p.Dd * 4);
    total = o;
  }
};


int vt_layernorm(hipStream_t stream, int M, int D, const float* in, const float* wb, float* out) {
  GS_KRANGE("vit_layernorm");
  hipLaunchKernelGGL(k_vit_layernorm, dim3((unsigned)((M + 3) / 4)), dim3(VT_T), 0, stream, M, D, in, wb, wb + D, out);
  GS_CHECK_LAUNCH("vit_layernorm");
  return MI355GS_OK;
}

int vt_attention(hipStream_t stream, int S, int N, int Wt, int P, int heads, const float* q, int ldq, const float* k, int ldk, const float* v,
                 int ldv, float* out, int ldo, const float* rope) {
  GS_KRANGE("vit_attention");
  hipLaunchKernelGGL(k_vit_attention, dim3((unsigned)((N + VT_AQ - 1) / VT_AQ), (unsigned)heads, (unsigned)S), dim3(VT_T), 0, stream, N, N, Wt, P,
                     q, ldq, k, ldk, v, ldv, out, ldo, rope);
  GS_CHECK_LAUNCH("vit_attention");
  return MI355GS_OK;
}

#define VT_TRY(call) do { const int rc_ = (call); if (rc_ != MI355GS_OK) return rc_; } while (0)

// x += attn(norm1(x)); x += mlp(norm2(x)) on M = S N rows; w: the block's weights
int vt_enc_block(hipStream_t stream, const VtPlan& p, int S, int Wt, int P, const float* w, const float* rope, float* x, float* t, float* qkv,
                 float* hid) {
  const int D = p.De, M = S * p.N;
  const float *n1 = w, *wqkv = n1 + 2 * D, *wproj = wqkv + VtPlan::lin(D, 3 * D), *n2 = wproj + VtPlan::lin(D, D), *fc1 = n2 + 2 * D,
              *fc2 = fc1 + VtPlan::lin(D, 4 * D);
  VT_TRY(vt_layernorm(stream, M, D, x, n1, t));
  VT_TRY(vt_gemm(stream, VT_PLAIN, M, D, 3 * D, t, wqkv, nullptr, qkv));
  VT_TRY(vt_attention(stream, S, p.N, Wt, P, p.He, qkv, 3 * D, qkv + D, 3 * D, qkv + 2 * D, 3 * D, t, D, rope));
  VT_TRY(vt_gemm(stream, VT_RESID, M, D, D, t, wproj, x, x));
  VT_TRY(vt_layernorm(stream, M, D, x, n2, t));
  VT_TRY(vt_gemm(stream, VT_GELU, M, D, 4 * D, t, fc1, nullptr, hid));
  VT_TRY(vt_gemm(stream, VT_RESID, M, 4 * D, D, hid, fc2, x, x));
  return MI355GS_OK;
}

// One side of one decoder layer (croco's DecoderBlock): xn = block(x, y) with x and y the previous layer's outputs, both left as
// they are (the other side reads them too).
int vt_dec_block(hipStream_t stream, const VtPlan& p, int S, int Wt, int P, const float* w, const float* rope, const float* x, const float* y,
                 float* xn, float* t, float* yn, float* qkv, float* hid) {
  const int D = p.Dd, M = S * p.N;
  const size_t plane = (size_t)M * D, dd = VtPlan::lin(D, D);
  const float *n1 = w, *wqkv = n1 + 2 * D, *wproj = wqkv + VtPlan::lin(D, 3 * D), *ny = wproj + dd, *n2 = ny + 2 * D, *wq = n2 + 2 * D,
              *wk = wq + dd, *wv = wk + dd, *wcp = wv + dd, *n3 = wcp + dd, *fc1 = n3 + 2 * D, *fc2 = fc1 + VtPlan::lin(D, 4 * D);
  VT_TRY(vt_layernorm(stream, M, D, x, n1, t));
  VT_TRY(vt_gemm(stream, VT_PLAIN, M, D, 3 * D, t, wqkv, nullptr, qkv));
  VT_TRY(vt_attention(stream, S, p.N, Wt, P, p.Hd, qkv, 3 * D, qkv + D, 3 * D, qkv + 2 * D, 3 * D, t, D, rope));
  VT_TRY(vt_gemm(stream, VT_RESID, M, D, D, t, wproj, x, xn));
  VT_TRY(vt_layernorm(stream, M, D, y, ny, yn));
  VT_TRY(vt_layernorm(stream, M, D, xn, n2, t));
  VT_TRY(vt_gemm(stream, VT_PLAIN, M, D, D, t, wq, nullptr, qkv));
  VT_TRY(vt_gemm(stream, VT_PLAIN, M, D, D, yn, wk, nullptr, qkv + plane));
  VT_TRY(vt_gemm(stream, VT_PLAIN, M, D, D, yn, wv, nullptr, qkv + 2 * plane));
  VT_TRY(vt_attention(stream, S, p.N, Wt, P, p.Hd, qkv, D, qkv + plane, D, qkv + 2 * plane, D, t, D, rope));
  VT_TRY(vt_gemm(stream, VT_RESID, M, D, D, t, wcp, xn, xn));
  VT_TRY(vt_layernorm(stream, M, D, xn, n3, t));
  VT_TRY(vt_gemm(stream, VT_GELU, M, D, 4 * D, t, fc1, nullptr, hid));
  VT_TRY(vt_gemm(stream, VT_RESID, M, 4 * D, D, hid, fc2, xn, xn));
  return MI355GS_OK;
}

bool vt_aligned(const void* a, const void* b, const void* c, const void* d) {
  return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0);
}

}  // namespace

extern "C" {

size_t mi355gs_vit_encode_scratch_bytes(const mi355gs_vit_config* cfg, int Ht, int Wt, int V) {
  const VtPlan p(cfg, Ht, Wt);
  if (!p.ok || V <= 0 || V > 256) return 0;
  return VtEncScratch(p, (size_t)V * p.N).total;
}

int mi355gs_vit_encode(void* stream_, const mi355gs_vit_config* cfg, const float* weights, const float* rope, int Ht, int Wt, int V,
                       const float* images, void* scratch, float* feat) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const VtPlan p(cfg, Ht, Wt);
  if (!p.ok || V <= 0 || V > 256 || !weights || !rope || !images || !scratch || !feat) return MI355GS_EINVAL;
  if (!vt_aligned(weights, images, scratch, feat) || ((uintptr_t)rope & 3)) return MI355GS_EINVAL;
  const int M = V * p.N, P = std::max(Ht, Wt);
  const VtEncScratch sl(p, (size_t)M);
  float* t = (float*)((char*)scratch + sl.t);
  float* qkv = (float*)((char*)scratch + sl.qkv);
  float* hid = (float*)((char*)scratch + sl.hid);

  const long long total4 = (long long)M * (VT_PATCH_K / 4);
  GS_KRANGE("vit_patches");
  hipLaunchKernelGGL(k_vit_patches, dim3((unsigned)((total4 + VT_T - 1) / VT_T)), dim3(VT_T), 0, stream, total4, Ht, Wt, images, hid);
  GS_CHECK_LAUNCH("vit_patches");
  const float* w = weights;
  VT_TRY(vt_gemm(stream, VT_PLAIN, M, VT_PATCH_K, p.De, hid, w, nullptr, feat));
  w += VtPlan::lin(VT_PATCH_K, p.De);
  for (int l = 0; l < p.Le; ++l, w += p.enc_block()) VT_TRY(vt_enc_block(stream, p, V, Wt, P, w, rope, feat, t, qkv, hid));
  return vt_layernorm(stream, M, p.De, feat, w, feat);
}

size_t mi355gs_vit_decode_scratch_bytes(const mi355gs_vit_config* cfg, int Ht, int Wt, int E) {
  const VtPlan p(cfg, Ht, Wt);
  if (!p.ok || E <= 0 || E > 65535) return 0;
  return VtDecScratch(p, (size_t)E).total;
}

int mi355gs_vit_decode(void* stream_, const mi355gs_vit_config* cfg, const float* weights, const float* rope, int Ht, int Wt, int V, int E,
                       const int32_t* edges, const float* feat, void* scratch, float* const out1[4], float* const out2[4]) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const VtPlan p(cfg, Ht, Wt);
  if (!p.ok || V <= 0 || V > 256 || E <= 0 || E > 65535 || !weights || !rope || !edges || !feat || !scratch || !out1 || !out2) return MI355GS_EINVAL;
  if (!vt_aligned(weights, feat, scratch, nullptr) || ((uintptr_t)rope & 3)) return MI355GS_EINVAL;
  for (int i = 0; i < 4; ++i)
    if (!out1[i] || !out2[i] || !vt_aligned(out1[i], out2[i], nullptr, nullptr)) return MI355GS_EINVAL;
  for (int i = 0; i < 2 * E; ++i)
    if (edges[i] < 0 || edges[i] >= V) return MI355GS_EINVAL;   // edges: host memory
  float* const* outs[2] = {out1, out2};
  const int M = E * p.N, P = std::max(Ht, Wt), D = p.Dd;
  const VtDecScratch sl(p, (size_t)E);
  char* sb = (char*)scratch;
  int32_t* d_edges = (int32_t*)(sb + sl.edges);
  float *t = (float*)(sb + sl.t), *yn = (float*)(sb + sl.yn), *qkv = (float*)(sb + sl.qkv), *hid = (float*)(sb + sl.hid);
  if (hipMemcpyAsync(d_edges, edges, (size_t)E * 2 * sizeof(int32_t), hipMemcpyHostToDevice, stream) != hipSuccess) return MI355GS_ELAUNCH;

  const float* w_embed = weights + p.dec_offset();
  const float* w_side[2] = {w_embed + VtPlan::lin(p.De, D), w_embed + VtPlan::lin(p.De, D) + p.Ld * p.dec_block()};
  const float* w_norm = w_side[1] + p.Ld * p.dec_block();
  float* cur[2];
  for (int s = 0; s < 2; ++s) {   // hook 0: the encoder rows of the side's image; layer 0's input: decoder_embed of them
    const long long total4 = (long long)M * (p.De / 4);
    GS_KRANGE("vit_gather");
    hipLaunchKernelGGL(k_vit_gather, dim3((unsigned)((total4 + VT_T - 1) / VT_T)), dim3(VT_T), 0, stream, total4, p.N * (p.De / 4), s,
                       (const int32_t*)d_edges, (const lp_f4*)feat, (lp_f4*)outs[s][0]);
    GS_CHECK_LAUNCH("vit_gather");
    cur[s] = (float*)(sb + sl.x[s][0]);
    VT_TRY(vt_gemm(stream, VT_PLAIN, M, p.De, D, outs[s][0], w_embed, nullptr, cur[s]));
  }
  for (int l = 1; l <= p.Ld; ++l) {
    float* nxt[2];
    for (int s = 0; s < 2; ++s) {
      // a hooked layer's output is written where the caller wants it; the last one passes through dec_norm first
      nxt[s] = l == p.hooks[1] ? outs[s][1] : l == p.hooks[2] ? outs[s][2] : (float*)(sb + sl.x[s][l & 1]);
      VT_TRY(vt_dec_block(stream, p, E, Wt, P, w_side[s] + (size_t)(l - 1) * p.dec_block(), rope, cur[s], cur[s ^ 1], nxt[s], t, yn, qkv, hid));
    }
    cur[0] = nxt[0]; cur[1] = nxt[1];
  }
  for (int s = 0; s < 2; ++s) VT_TRY(vt_layernorm(stream, M, D, cur[s], w_norm, outs[s][3]));
  return MI355GS_OK;
}

}  // extern "C"
