// MASt3R's dense heads on the device (include/mi355gs.h, mi355gs_dpt_head / mi355gs_local_features): the DPT head that turns the
// four hooked token tensors of one side (mi355gs_vit_decode's outputs, as they are) into a pointmap and a confidence per pixel
// (dust3r/heads/dpt_head.py for the order of operations, dust3r/heads/postprocess.py for the last step), and the local-feature
// MLP of mast3r/catmlp_dpt_head.py.  float32 throughout, activations channels-last [edge][y][x][channel].
//
//   k_vit_gemm     (mm_tile.h) every 1 x 1 convolution, both ConvTransposes (a GEMM to [row][s s C]) and the MLP
//   k_dpt_scatter  the ConvTranspose's store: [token][(dy s + dx) C + c] -> pixel (s y + dy, s x + dx), one float4 per thread
//   k_dpt_conv     3 x 3 implicit GEMM on the shared K loop and tap fetch (mm_tile.h), as k_lpips_conv: 128 output pixels x (32, 64
//                  or 128) outputs per workgroup.  Switches: ReLU on the staged input, bias or none, stride 1 or 2, up to two
//                  residual tensors added in the epilogue.
//   k_dpt_up2      bilinear x 2, align_corners = True, one float4 of channels per thread; its output size may be smaller than
//                  twice the input (refinenet4's crop: the steps behind it are per pixel, so the crop is taken here)
//   k_dpt_final    head.2 (3 x 3, F / 2 -> last_dim) with every output channel of its 128 pixels in one workgroup; the epilogue
//                  applies ReLU, multiplies by head.4 (last_dim -> 4, padded to 32 columns, through the matrix helper) and runs
//                  postprocess: 16 bytes per pixel leave the kernel.
//   k_dpt_concat   cat(hook 0, hook 3) per token;  k_dpt_desc: pixel_shuffle(16), the descriptor's norm, its confidence.
// No atomics, no memset, no allocation, no host synchronisation; equal bits run to run, and a pixel's result does not depend on
// how many edges share the call (every row of a tile is an independent k-ordered chain).
#include "common.h"
#include "mm_tile.h"

namespace {

constexpr int DP_T = 256;            // threads of the small kernels
constexpr int DP_MAX_TOKENS = 4096;
constexpr int DP_NTAPS = 8;          // intermediates a call leaves in its scratch: L0..L3, path_4..path_1

// ---------------------------------------------------------------------------------------------------- 3 x 3 convolution
// grid (ceil(P / 128), Cout / (32 NT)).  in [edge][Hi][Wi][Cin], out [edge][Ho][Wo][Cout]; Cin, Cout multiples of 32; wt
// [(3 ky + kx) Cin + ci][Cout].  out = r2 + (r1 + (conv + bias)), each of bias, r1, r2 where given (r2 only with r1).
template <int NT>
__global__ __launch_bounds__(MM_T) void k_dpt_conv(MmConv g, const float* __restrict__ in, const float* __restrict__ wt,
                                                   const float* __restrict__ bias, const float* __restrict__ r1, const float* __restrict__ r2,
                                                   float* __restrict__ out) {
  constexpr int LDB = mm_ldb(NT, false);
  __shared__ lp_f4 As4[MM_BM * MM_LDA / 4];
  __shared__ lp_f4 Bs4[MM_BK * LDB / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile0 = blockIdx.x * MM_BM, n0 = blockIdx.y * 32 * NT;
  const MmTapFetch<false> fetch(g, in);
  mm_k_loop<NT, LDB>(fetch.nq, wt, g.Cout, n0, (float*)As4, (float*)Bs4, fetch, [&](lp_acc16 (&acc)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + 32 * j + (lane & 31);
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = tile0 + 32 * wave + lp_acc_row(r, lane);
        if (p < g.P) {
          const size_t o = (size_t)p * g.Cout + n;
          float y = acc[j][r] + bv;
          if (r1) y = r1[o] + y;
          if (r2) y = r2[o] + y;
          out[o] = y;
        }
      }
    }
  });
}

// ---------------------------------------------------------------------------------------------------- the last stage
struct DpPost { float conf_vmin, conf_span; };   // conf = vmin + min(exp(c3), span), span = vmax - vmin

// grid (ceil(P / 128)).  g.Cout = 32 NT = last_dim.  w4: head.4 as [last_dim][32] (columns 4.. zero) then its bias [32].
// pts3d [P][3], conf [P]; raw4 (may be null) [P][4]: the four channels before postprocess.
template <int NT>
__global__ __launch_bounds__(MM_T) void k_dpt_final(MmConv g, DpPost post, const float* __restrict__ in, const float* __restrict__ wt,
                                                    const float* __restrict__ bias, const float* __restrict__ w4, float* __restrict__ pts3d,
                                                    float* __restrict__ conf, float* __restrict__ raw4) {
  constexpr int BN = 32 * NT, LDB = mm_ldb(NT, false);
  __shared__ lp_f4 As4[MM_BM * MM_LDA / 4];
  __shared__ lp_f4 Bs4[MM_BK * LDB / 4];   // 32 LDB >= 32 x 32 NT floats: head.4's padded matrix fits
  float *As = (float*)As4, *Bs = (float*)Bs4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile0 = blockIdx.x * MM_BM;
  const MmTapFetch<true> fetch(g, in);
  mm_k_loop<NT, LDB>(fetch.nq, wt, g.Cout, 0, As, Bs, fetch, [&](lp_acc16 (&acc)[NT]) {
    __syncthreads();   // the last chunk has been consumed: both tiles are free
    for (int f = tid; f < BN * 8; f += MM_T) Bs4[f] = ((const lp_f4*)w4)[f];
    float* Aw = As + 32 * wave * MM_LDA;   // this wave's 32 pixels x 32 channels
    lp_acc16 o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float bv = bias[32 * j + (lane & 31)];
#pragma unroll
      for (int r = 0; r < 16; ++r) Aw[lp_acc_row(r, lane) * MM_LDA + (lane & 31)] = fmaxf(acc[j][r] + bv, 0.f);
      __syncthreads();
#pragma unroll 4
      for (int kk = 0; kk < 16; ++kk) lp_mfma_32x32x2(o, Aw + 2 * kk, MM_LDA, Bs + (32 * j + 2 * kk) * 32, 32, lane);
      __syncthreads();
    }
    if ((lane & 31) < 4) {
      const float b4 = w4[BN * 32 + (lane & 31)];
#pragma unroll
      for (int r = 0; r < 16; ++r) Aw[lp_acc_row(r, lane) * MM_LDA + (lane & 31)] = o[r] + b4;
    }
    __syncthreads();
    const int p = tile0 + 32 * wave + lane;
    if (lane < 32 && p < g.P) {
      const float x = Aw[lane * MM_LDA], y = Aw[lane * MM_LDA + 1], z = Aw[lane * MM_LDA + 2], c = Aw[lane * MM_LDA + 3];
      if (raw4) {
        const lp_f4 v = {x, y, z, c};
        *(lp_f4*)(raw4 + (size_t)p * 4) = v;
      }
      const float d = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
      const float s = expm1f(d) / fmaxf(d, 1e-8f);   // xyz / max(d, 1e-8) * expm1(d); d = 0: 0 / 1e-8 = 0, no 0 / 0
      pts3d[(size_t)p * 3] = x * s;
      pts3d[(size_t)p * 3 + 1] = y * s;
      pts3d[(size_t)p * 3 + 2] = z * s;
      conf[p] = post.conf_vmin + fminf(expf(c), post.conf_span);
    }
  });
}

// ---------------------------------------------------------------------------------------------------- small kernels
// in [rows][s s C] (rows = edge, y, x of the Ht x Wt grid) -> out [edge][s Ht][s Wt][C]; one float4 per thread of out
__global__ __launch_bounds__(DP_T) void k_dpt_scatter(long long total4, int Ht, int Wt, int s, int C4, const lp_f4* __restrict__ in,
                                                      lp_f4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * DP_T + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)(i % C4);
  long long r = i / C4;
  const int X = (int)(r % (s * Wt));
  r /= s * Wt;
  const int Y = (int)(r % (s * Ht));
  const long long e = r / (s * Ht);
  const int y = Y / s, dy = Y - y * s, x = X / s, dx = X - x * s;
  out[i] = in[(((size_t)e * Ht + y) * Wt + x) * (size_t)(s * s * C4) + (size_t)(dy * s + dx) * C4 + c];
}

// bilinear x 2, align_corners = True: in [edge][hi][wi][C] -> out [edge][ho][wo][C], ho <= 2 hi, wo <= 2 wi (a crop of the
// full result).  sy = (hi - 1) / (2 hi - 1) (0 when hi = 1), sx likewise: src = dst * scale, i0 = floor(src), i1 = min(i0 + 1, in - 1).
__global__ __launch_bounds__(DP_T) void k_dpt_up2(long long total4, int hi, int wi, int ho, int wo, int C4, float sy, float sx,
                                                  const lp_f4* __restrict__ in, lp_f4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * DP_T + threadIdx.x;
  if (i >= total4) return;
  const int c = (int)(i % C4);
  long long r = i / C4;
  const int X = (int)(r % wo);
  r /= wo;
  const int Y = (int)(r % ho);
  const long long e = r / ho;
  const float fy = (float)Y * sy, fx = (float)X * sx;
  const int y0 = min((int)floorf(fy), hi - 1), x0 = min((int)floorf(fx), wi - 1);
  const int y1 = min(y0 + 1, hi - 1), x1 = min(x0 + 1, wi - 1);
  const float ly = fy - (float)y0, lx = fx - (float)x0;
  const lp_f4* src = in + (size_t)e * hi * wi * C4 + c;
  const lp_f4 a = src[((size_t)y0 * wi + x0) * C4], b = src[((size_t)y0 * wi + x1) * C4];
  const lp_f4 cc = src[((size_t)y1 * wi + x0) * C4], d = src[((size_t)y1 * wi + x1) * C4];
  lp_f4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    LP_AT(v, k) = (1.f - ly) * ((1.f - lx) * LP_ATC(a, k) + lx * LP_ATC(b, k)) + ly * ((1.f - lx) * LP_ATC(cc, k) + lx * LP_ATC(d, k));
  out[i] = v;
}

// out[row] = cat(a[row][0..Ka), b[row][0..Kb)); one float4 per thread
__global__ __launch_bounds__(DP_T) void k_dpt_concat(long long total4, int Ka4, int Kb4, const lp_f4* __restrict__ a, const lp_f4* __restrict__ b,
                                                     lp_f4* __restrict__ out) {
  const long long i = (long long)blockIdx.x * DP_T + threadIdx.x;
  if (i >= total4) return;
  const int K4 = Ka4 + Kb4, c = (int)(i % K4);
  const long long row = i / K4;
  out[i] = c < Ka4 ? a[(size_t)row * Ka4 + c] : b[(size_t)row * Kb4 + (c - Ka4)];
}

// feat [edge][Ht Wt][(D + two) 256] -> desc [edge][16 Ht][16 Wt][D] (channel c of pixel (16 ty + py, 16 tx + px) is feature
// c 256 + 16 py + px: pixel_shuffle(16)), divided by its norm; desc_conf (may be null) = vmin + min(exp(channel D), span).
// One thread per pixel, px fastest: a wave's reads of one channel are contiguous.
__global__ __launch_bounds__(DP_T) void k_dpt_desc(long long total, int Ht, int Wt, int D, int NF, DpPost post, const float* __restrict__ feat,
                                                   float* __restrict__ desc, float* __restrict__ desc_conf) {
  const long long i = (long long)blockIdx.x * DP_T + threadIdx.x;
  if (i >= total) return;
  const int sub = (int)(i & 255), py = sub >> 4, px = sub & 15;
  const long long tok = i >> 8;
  const int n = (int)(tok % (Ht * Wt));
  const long long e = tok / (Ht * Wt);
  const int ty = n / Wt, tx = n - ty * Wt;
  const float* src = feat + (size_t)tok * NF + sub;
  float ss = 0.f;
  for (int c = 0; c < D; ++c) ss = fmaf(src[c * 256], src[c * 256], ss);
  const float nrm = sqrtf(ss);
  const size_t p = ((size_t)e * (16 * Ht) + 16 * ty + py) * (size_t)(16 * Wt) + 16 * tx + px;
  float* dst = desc + p * D;
  for (int c = 0; c < D; ++c) dst[c] = src[c * 256] / nrm;
  if (desc_conf) desc_conf[p] = post.conf_vmin + fminf(expf(src[D * 256]), post.conf_span);
}

// ---------------------------------------------------------------------------------------------------- host side
size_t dp_lin(int K, int N) { return (size_t)K * N + N; }

struct DpPlan {
  bool ok = false;
  int Ht, Wt, N, E, F, F2, LD;
  int ct[4], ld[4];
  int h[4], w[4];       // L0..L3: 4x, 2x, 1x, ceil(1/2) of the token grid
  int H, W;
  DpPlan(const mi355gs_dpt_config* c, int Ht_, int Wt_, int E_) {
    if (!c || Ht_ <= 0 || Wt_ <= 0 || (long long)Ht_ * Wt_ > DP_MAX_TOKENS || E_ <= 0 || E_ > 65535) return;
    Ht = Ht_; Wt = Wt_; N = Ht * Wt; E = E_;
    F = c->feature_dim; F2 = F / 2; LD = c->last_dim;
    if (F < 64 || F > 256 || F % 64 || LD < 32 || LD > 128 || LD % 32) return;   // F / 2 a multiple of 32, at most 128
    for (int k = 0; k < 4; ++k) {
      ct[k] = c->dim_tokens[k]; ld[k] = c->layer_dims[k];
      if (ct[k] < 32 || ct[k] > 4096 || ct[k] % 32 || ld[k] < 32 || ld[k] > 1024 || ld[k] % 32) return;
    }
    if (!(c->conf_vmax > c->conf_vmin)) return;
    H = 16 * Ht; W = 16 * Wt;
    if ((long long)E * H * W > 0x7fffffffLL / 4) return;   // a pixel's index, times 4, is an int
    h[0] = 4 * Ht; w[0] = 4 * Wt; h[1] = 2 * Ht; w[1] = 2 * Wt; h[2] = Ht; w[2] = Wt; h[3] = (Ht + 1) / 2; w[3] = (Wt + 1) / 2;
    ok = true;
  }
  // the blob (include/mi355gs.h), in floats
  size_t rcu() const { return 2 * dp_lin(9 * F, F); }
};

struct DpScratch {
  size_t gemm, gemm2, act[4], tap[DP_NTAPS], t1, t2, t3, up, h0, total;
  DpScratch(const DpPlan& p) {
    const size_t E = p.E, N = p.N, F = p.F;
    size_t o = 256;   // no buffer at offset 0: 0 is the tap query's refusal
    size_t g = 0;
    for (int k = 0; k < 4; ++k) g = std::max(g, E * N * (size_t)p.ld[k]);
    gemm = o; o += gs_align(g * 4);
    gemm2 = o; o += gs_align(E * N * std::max((size_t)16 * p.ld[0], (size_t)4 * p.ld[1]) * 4);
    for (int k = 0; k < 4; ++k) { act[k] = o; o += gs_align(E * p.h[k] * p.w[k] * (size_t)p.ld[k] * 4); }
    for (int k = 0; k < 4; ++k) { tap[k] = o; o += gs_align(E * p.h[k] * p.w[k] * F * 4); }
    // path_4 (L2's size), path_3 (L1's), path_2 (L0's), path_1 (8 Ht x 8 Wt)
    tap[4] = o; o += gs_align(E * p.h[2] * p.w[2] * F * 4);
    tap[5] = o; o += gs_align(E * p.h[1] * p.w[1] * F * 4);
    tap[6] = o; o += gs_align(E * p.h[0] * p.w[0] * F * 4);
    tap[7] = o; o += gs_align(E * 64 * N * F * 4);
    const size_t big = E * 16 * N * F * 4;   // L0's size: the largest input of a fusion block
    t1 = o; o += gs_align(big);
    t2 = o; o += gs_align(big);
    t3 = o; o += gs_align(big);
    up = o; o += gs_align(E * 256 * N * (size_t)p.F2 * 4);   // every upsampled tensor; the largest is the head's, H x W x F / 2
    h0 = o; o += gs_align(E * 64 * N * (size_t)p.F2 * 4);
    total = o;
  }
};

#define DP_TRY(call) do { const int rc_ = (call); if (rc_ != MI355GS_OK) return rc_; } while (0)

// NT of a 3 x 3 convolution: 128 outputs per workgroup where Cout allows, else 64, else 32
int dp_conv_nt(int Cout) { return Cout % 128 == 0 ? 4 : Cout % 64 == 0 ? 2 : 1; }

int dp_conv(hipStream_t stream, int E, int Hi, int Wi, int stride, bool relu_in, int Cin, int Cout, const float* in, const float* wt, bool has_bias,
            const float* r1, const float* r2, float* out) {
  const int Ho = (Hi + stride - 1) / stride, Wo = (Wi + stride - 1) / stride;
  const MmConv g = {E * Ho * Wo, Hi, Wi, Ho, Wo, Cin, Cout, stride, relu_in ? 1 : 0};
  const float* bias = has_bias ? wt + (size_t)9 * Cin * Cout : nullptr;
  const int nt = dp_conv_nt(Cout);
  const dim3 grid((unsigned)((g.P + MM_BM - 1) / MM_BM), (unsigned)(Cout / (32 * nt)));
  GS_KRANGE("dpt_conv");
  switch (nt) {
    case 4: hipLaunchKernelGGL(k_dpt_conv<4>, grid, dim3(MM_T), 0, stream, g, in, wt, bias, r1, r2, out); break;
    case 2: hipLaunchKernelGGL(k_dpt_conv<2>, grid, dim3(MM_T), 0, stream, g, in, wt, bias, r1, r2, out); break;
    default: hipLaunchKernelGGL(k_dpt_conv<1>, grid, dim3(MM_T), 0, stream, g, in, wt, bias, r1, r2, out); break;
  }
  GS_CHECK_LAUNCH("dpt_conv");
  return MI355GS_OK;
}

int dp_up2(hipStream_t stream, int E, int hi, int wi, int ho, int wo, int C, const float* in, float* out) {
  const long long total4 = (long long)E * ho * wo * (C / 4);
  const float sy = hi > 1 ? (float)(hi - 1) / (float)(2 * hi - 1) : 0.f, sx = wi > 1 ? (float)(wi - 1) / (float)(2 * wi - 1) : 0.f;
  GS_KRANGE("dpt_up2");
  hipLaunchKernelGGL(k_dpt_up2, dim3((unsigned)((total4 + DP_T - 1) / DP_T)), dim3(DP_T), 0, stream, total4, hi, wi, ho, wo, C / 4, sy, sx,
                     (const lp_f4*)in, (lp_f4*)out);
  GS_CHECK_LAUNCH("dpt_up2");
  return MI355GS_OK;
}

// x + conv2(relu(conv1(relu(x)))), plus `also` where given: out = also + (x + ...)
int dp_rcu(hipStream_t stream, const DpPlan& p, int h, int w, const float* wts, const float* x, const float* also, float* tmp, float* out) {
  DP_TRY(dp_conv(stream, p.E, h, w, 1, true, p.F, p.F, x, wts, true, nullptr, nullptr, tmp));
  return dp_conv(stream, p.E, h, w, 1, true, p.F, p.F, tmp, wts + dp_lin(9 * p.F, p.F), true, x, also, out);
}

// FeatureFusionBlock(a[, b]) on h x w, its upsampled result cropped to ho x wo -> path.  wts: [rcu1 when b], rcu2, out_conv.
int dp_fusion(hipStream_t stream, const DpPlan& p, const DpScratch& sl, char* sb, int h, int w, int ho, int wo, const float* wts, const float* a,
              const float* b, float* path) {
  float *t1 = (float*)(sb + sl.t1), *t2 = (float*)(sb + sl.t2), *t3 = (float*)(sb + sl.t3), *up = (float*)(sb + sl.up);
  const float* o = a;
  if (b) {
    DP_TRY(dp_rcu(stream, p, h, w, wts, b, a, t1, t2));   // a + resConfUnit1(b)
    wts += p.rcu();
    o = t2;
  }
  DP_TRY(dp_rcu(stream, p, h, w, wts, o, nullptr, t1, t3));
  wts += p.rcu();
  DP_TRY(dp_up2(stream, p.E, h, w, ho, wo, p.F, t3, up));
  return vt_gemm<true>(stream, VT_PLAIN, p.E * ho * wo, p.F, p.F, up, wts, nullptr, path);
}

bool dp_aligned(const void* a, const void* b, const void* c, const void* d) {
  return ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0);
}

struct DpMlp {
  bool ok = false;
  int Ka, Kb, hid, D, two, NF, Ht, Wt, E;
  DpMlp(const mi355gs_dpt_config* c, int Ht_, int Wt_, int E_) {
    if (!c || Ht_ <= 0 || Wt_ <= 0 || (long long)Ht_ * Wt_ > DP_MAX_TOKENS || E_ <= 0 || E_ > 65535) return;
    Ht = Ht_; Wt = Wt_; E = E_;
    Ka = c->dim_tokens[0]; Kb = c->dim_tokens[3]; hid = c->mlp_hidden; D = c->local_feat_dim; two = c->two_confs ? 1 : 0;
    if (Ka < 32 || Ka > 4096 || Ka % 32 || Kb < 32 || Kb > 4096 || Kb % 32 || hid < 32 || hid > 32768 || hid % 32 || D < 1 || D > 255) return;
    if (!(c->desc_conf_vmax > c->desc_conf_vmin)) return;
    NF = (D + two) * 256;
    if ((long long)E * Ht * Wt * 256 * D > 0x7fffffffLL * 4) return;
    ok = true;
  }
  size_t M() const { return (size_t)E * Ht * Wt; }
  size_t cat_bytes() const { return gs_align(M() * (Ka + Kb) * 4); }
  size_t hid_bytes() const { return gs_align(M() * hid * 4); }
  size_t out_bytes() const { return gs_align(M() * NF * 4); }
};

}  // namespace

extern "C" {

size_t mi355gs_dpt_head_scratch_bytes(const mi355gs_dpt_config* cfg, int Ht, int Wt, int E) {
  const DpPlan p(cfg, Ht, Wt, E);
  return p.ok ? DpScratch(p).total : 0;
}

size_t mi355gs_dpt_head_tap_offset(const mi355gs_dpt_config* cfg, int Ht, int Wt, int E, int which) {
  const DpPlan p(cfg, Ht, Wt, E);
  if (!p.ok || which < 0 || which >= DP_NTAPS) return 0;
  return DpScratch(p).tap[which];
}

int mi355gs_dpt_head(void* stream_, const mi355gs_dpt_config* cfg, const float* weights, int Ht, int Wt, int E, const float* const hooks[4],
                     void* scratch, float* pts3d, float* conf, float* raw4) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const DpPlan p(cfg, Ht, Wt, E);
  if (!p.ok || !weights || !hooks || !scratch || !pts3d || !conf) return MI355GS_EINVAL;
  if (!dp_aligned(weights, scratch, raw4, nullptr) || (((uintptr_t)pts3d | (uintptr_t)conf) & 3)) return MI355GS_EINVAL;
  for (int k = 0; k < 4; ++k)
    if (!hooks[k] || !dp_aligned(hooks[k], nullptr, nullptr, nullptr)) return MI355GS_EINVAL;
  const DpScratch sl(p);
  char* sb = (char*)scratch;
  float *g1 = (float*)(sb + sl.gemm), *g2 = (float*)(sb + sl.gemm2);
  float* act[4];
  float* tap[DP_NTAPS];
  for (int k = 0; k < 4; ++k) act[k] = (float*)(sb + sl.act[k]);
  for (int k = 0; k < DP_NTAPS; ++k) tap[k] = (float*)(sb + sl.tap[k]);
  const int M = E * p.N, F = p.F;
  const float* w = weights;

  // act_postprocess
  for (int k = 0; k < 4; ++k) {
    const int C = p.ld[k];
    float* first = k == 2 ? act[2] : g1;
    DP_TRY(vt_gemm<true>(stream, VT_PLAIN, M, p.ct[k], C, hooks[k], w, nullptr, first));
    w += dp_lin(p.ct[k], C);
    if (k < 2) {
      const int s = k == 0 ? 4 : 2;
      DP_TRY(vt_gemm<true>(stream, VT_PLAIN, M, C, s * s * C, g1, w, nullptr, g2));
      w += dp_lin(C, s * s * C);
      const long long total4 = (long long)M * s * s * (C / 4);
      GS_KRANGE("dpt_scatter");
      hipLaunchKernelGGL(k_dpt_scatter, dim3((unsigned)((total4 + DP_T - 1) / DP_T)), dim3(DP_T), 0, stream, total4, Ht, Wt, s, C / 4,
                         (const lp_f4*)g2, (lp_f4*)act[k]);
      GS_CHECK_LAUNCH("dpt_scatter");
    } else if (k == 3) {
      DP_TRY(dp_conv(stream, E, Ht, Wt, 2, false, C, C, g1, w, true, nullptr, nullptr, act[3]));
      w += dp_lin(9 * C, C);
    }
  }
  // layer_rn: no bias
  for (int k = 0; k < 4; ++k) {
    DP_TRY(dp_conv(stream, E, p.h[k], p.w[k], 1, false, p.ld[k], F, act[k], w, false, nullptr, nullptr, tap[k]));
    w += (size_t)9 * p.ld[k] * F;
  }
  // refinenet4 (one input; cropped to L2's size), 3, 2, 1
  const size_t fuse1 = p.rcu() + dp_lin(F, F), fuse2 = 2 * p.rcu() + dp_lin(F, F);
  DP_TRY(dp_fusion(stream, p, sl, sb, p.h[3], p.w[3], p.h[2], p.w[2], w, tap[3], nullptr, tap[4]));
  w += fuse1;
  DP_TRY(dp_fusion(stream, p, sl, sb, p.h[2], p.w[2], p.h[1], p.w[1], w, tap[4], tap[2], tap[5]));
  w += fuse2;
  DP_TRY(dp_fusion(stream, p, sl, sb, p.h[1], p.w[1], p.h[0], p.w[0], w, tap[5], tap[1], tap[6]));
  w += fuse2;
  DP_TRY(dp_fusion(stream, p, sl, sb, p.h[0], p.w[0], 8 * Ht, 8 * Wt, w, tap[6], tap[0], tap[7]));
  w += fuse2;
  // head
  float *h0 = (float*)(sb + sl.h0), *up = (float*)(sb + sl.up);
  DP_TRY(dp_conv(stream, E, 8 * Ht, 8 * Wt, 1, false, F, p.F2, tap[7], w, true, nullptr, nullptr, h0));
  w += dp_lin(9 * F, p.F2);
  DP_TRY(dp_up2(stream, E, 8 * Ht, 8 * Wt, p.H, p.W, p.F2, h0, up));
  const MmConv g = {E * p.H * p.W, p.H, p.W, p.H, p.W, p.F2, p.LD, 1, 0};   // k_dpt_final's MmTapFetch<true> needs Ho = Hi, Wo = Wi, stride 1, no ReLU
  const float* b2 = w + (size_t)9 * p.F2 * p.LD;
  const float* w4 = b2 + p.LD;
  const DpPost post = {cfg->conf_vmin, cfg->conf_vmax - cfg->conf_vmin};
  const dim3 grid((unsigned)((g.P + MM_BM - 1) / MM_BM));
  GS_KRANGE("dpt_final");
  switch (p.LD / 32) {
    case 4: hipLaunchKernelGGL(k_dpt_final<4>, grid, dim3(MM_T), 0, stream, g, post, (const float*)up, w, b2, w4, pts3d, conf, raw4); break;
    case 3: hipLaunchKernelGGL(k_dpt_final<3>, grid, dim3(MM_T), 0, stream, g, post, (const float*)up, w, b2, w4, pts3d, conf, raw4); break;
    case 2: hipLaunchKernelGGL(k_dpt_final<2>, grid, dim3(MM_T), 0, stream, g, post, (const float*)up, w, b2, w4, pts3d, conf, raw4); break;
    default: hipLaunchKernelGGL(k_dpt_final<1>, grid, dim3(MM_T), 0, stream, g, post, (const float*)up, w, b2, w4, pts3d, conf, raw4); break;
  }
  GS_CHECK_LAUNCH("dpt_final");
  return MI355GS_OK;
}

size_t mi355gs_local_features_scratch_bytes(const mi355gs_dpt_config* cfg, int Ht, int Wt, int E) {
  const DpMlp m(cfg, Ht, Wt, E);
  return m.ok ? m.cat_bytes() + m.hid_bytes() + m.out_bytes() : 0;
}

int mi355gs_local_features(void* stream_, const mi355gs_dpt_config* cfg, const float* weights, int Ht, int Wt, int E, const float* hook0,
                           const float* hook3, void* scratch, float* desc, float* desc_conf) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const DpMlp m(cfg, Ht, Wt, E);
  if (!m.ok || !weights || !hook0 || !hook3 || !scratch || !desc || (m.two && !desc_conf)) return MI355GS_EINVAL;
  if (!dp_aligned(weights, hook0, hook3, scratch) || (((uintptr_t)desc | (uintptr_t)desc_conf) & 3)) return MI355GS_EINVAL;
  char* sb = (char*)scratch;
  float *cat = (float*)sb, *hid = (float*)(sb + m.cat_bytes()), *out = (float*)(sb + m.cat_bytes() + m.hid_bytes());
  const int M = (int)m.M(), K = m.Ka + m.Kb;
  const long long total4 = (long long)M * (K / 4);
  GS_KRANGE("dpt_concat");
  hipLaunchKernelGGL(k_dpt_concat, dim3((unsigned)((total4 + DP_T - 1) / DP_T)), dim3(DP_T), 0, stream, total4, m.Ka / 4, m.Kb / 4,
                     (const lp_f4*)hook0, (const lp_f4*)hook3, (lp_f4*)cat);
  GS_CHECK_LAUNCH("dpt_concat");
  DP_TRY(vt_gemm<true>(stream, VT_GELU, M, K, m.hid, cat, weights, nullptr, hid));
  DP_TRY(vt_gemm<true>(stream, VT_PLAIN, M, m.hid, m.NF, hid, weights + dp_lin(K, m.hid), nullptr, out));
  const long long total = (long long)M * 256;
  const DpPost post = {cfg->desc_conf_vmin, cfg->desc_conf_vmax - cfg->desc_conf_vmin};
  GS_KRANGE("dpt_desc");
  hipLaunchKernelGGL(k_dpt_desc, dim3((unsigned)((total + DP_T - 1) / DP_T)), dim3(DP_T), 0, stream, total, Ht, Wt, m.D, m.NF, post,
                     (const float*)out, desc, m.two ? desc_conf : nullptr);
  GS_CHECK_LAUNCH("dpt_desc");
  return MI355GS_OK;
}

}  // extern "C"
