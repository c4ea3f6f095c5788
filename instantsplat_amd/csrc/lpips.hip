// LPIPS (VGG16) of 8-bit frame pairs on the device (include/mi355gs.h, mi355gs_lpips_vgg_rgb8): the reference's
// lpipsPyTorch/modules/{lpips,networks,utils}.py forward for the `vgg` net, float32 throughout.
//
// Both stacks go through the network as ONE batch of 2N images (a's frames, then b's), flattened to P = 2 N H W pixels.
// Activations are channels-last float32, [pixel][channel], in two ping-pong buffers of the caller's scratch; a convolution is
// the implicit GEMM  out[p][co] = relu(bias[co] + sum_k in[p + offset(tap)][ci] w[k][co]),  k = tap * Cin + ci  (tap = 3 ky + kx),
// so K is contiguous in memory per tap and the packed weights are a plain [K][Cout] matrix.
//
//   k_lpips_conv0   bytes -> block 1's first layer.  K = 27: VALU, the normalised 3x3 patches of 64 pixels staged in LDS.
//   k_lpips_conv    every other layer: 128 pixels x (32, 64, 96 or 128) outputs per workgroup on the shared K loop and tap fetch
//                   (mm_tile.h: v_mfma_f32_32x32x2_f32, exact float32, a k-ordered fmaf chain), bias + ReLU in the epilogue.
//   k_lpips_pool    2x2 stride-2 max-pool (floor) in front of blocks 2 to 5.
//   k_lpips_tap     per pixel of a pair: channel-normalise both, sum_c w_c (xa^ - xb^)^2; per-workgroup partial sums in a fixed order.
//   k_lpips_finish  per pair: the five spatial means and their sum, fixed order.  No atomics anywhere: equal bits run to run, and
//                   (a, b) against (b, a) — the difference is squared and every other step treats the two images alike.
#include "common.h"
#include "mm_tile.h"

namespace {

constexpr int LP_T = 256;            // threads of every workgroup but the convolution's (mm_tile.h) and the finishing one
constexpr int LP_P0 = 64;            // pixels of a first-layer tile
constexpr int LP_TAP_PIX = 256;      // pixels of a tap workgroup: 4 waves x 64
constexpr int LP_MAX_C = 512;
constexpr float LP_EPS = 1e-10f;

// ---------------------------------------------------------------------------------------------------- first layer
// (byte / 255 - mean) / std as the reference's float32 tensor ops round it; the zero padding pads the NORMALISED image.
__global__ __launch_bounds__(LP_T) void k_lpips_conv0(int N, int H, int W, int C, const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                      const float* __restrict__ wt, const float* __restrict__ bias, float* __restrict__ out) {
  __shared__ float patch[LP_P0 * 27];
  const int tid = threadIdx.x;
  const long long HW = (long long)H * W, P = 2 * (long long)N * HW;
  const long long tile0 = (long long)blockIdx.x * LP_P0;
  for (int e = tid; e < LP_P0 * 27; e += LP_T) {
    const int m = e / 27, k = e - m * 27, t = k / 3, c = k - t * 3;
    const long long p = tile0 + m;
    float v = 0.f;
    if (p < P) {
      const long long img = p / HW, rem = p - img * HW;
      const int y = (int)(rem / W) + t / 3 - 1, x = (int)(rem % W) + t % 3 - 1;
      if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
        const uint8_t* src = img < N ? a + (size_t)img * (size_t)(3 * HW) : b + (size_t)(img - N) * (size_t)(3 * HW);
        const float mean = c == 0 ? -.030f : c == 1 ? -.088f : -.188f;
        const float sd = c == 0 ? .458f : c == 1 ? .448f : .450f;
        v = ((float)src[((size_t)y * W + x) * 3 + c] / 255.0f - mean) / sd;
      }
    }
    patch[e] = v;
  }
  __syncthreads();
  const int co = blockIdx.y * 32 + (tid & 31), pg = tid >> 5;
  float w[27];
#pragma unroll
  for (int k = 0; k < 27; ++k) w[k] = wt[k * C + co];
  const float bv = bias[co];
  for (int s = 0; s < LP_P0 / 8; ++s) {
    const int m = pg + 8 * s;
    const long long p = tile0 + m;
    if (p >= P) break;
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) acc = fmaf(patch[m * 27 + k], w[k], acc);
    out[(size_t)p * C + co] = fmaxf(acc + bv, 0.f);
  }
}

// ---------------------------------------------------------------------------------------------------- implicit GEMM
// grid (ceil(P / 128), Cout / (32 NT)).  P = images x H x W flattened pixels of [image][y][x][Cin] input; Cin, Cout multiples of 32.
// The shared tap fetch at stride 1 without ReLU on the way in (mm_tile.h); bias + ReLU in the epilogue.
template <int NT>
__global__ __launch_bounds__(MM_T) void k_lpips_conv(int P, int H, int W, int Cin, int Cout, const float* __restrict__ in,
                                                     const float* __restrict__ wt, const float* __restrict__ bias, float* __restrict__ out) {
  constexpr int LDB = mm_ldb(NT, false);
  __shared__ lp_f4 As4[MM_BM * MM_LDA / 4];
  __shared__ lp_f4 Bs4[MM_BK * LDB / 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile0 = blockIdx.x * MM_BM, n0 = blockIdx.y * 32 * NT;
  const MmConv g = {P, H, W, H, W, Cin, Cout, 1, 0};
  const MmTapFetch<true> fetch(g, in);
  mm_k_loop<NT, LDB>(fetch.nq, wt, Cout, n0, (float*)As4, (float*)Bs4, fetch, [&](lp_acc16 (&acc)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + 32 * j + (lane & 31);
      const float bv = bias[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int p = tile0 + 32 * wave + lp_acc_row(r, lane);
        if (p < P) out[(size_t)p * Cout + n] = fmaxf(acc[j][r] + bv, 0.f);
      }
    }
  });
}

// ---------------------------------------------------------------------------------------------------- max-pool
// [images][H][W][C] -> [images][H / 2][W / 2][C], one float4 of channels per thread
__global__ __launch_bounds__(LP_T) void k_lpips_pool(long long total4, int H, int W, int C4, const float4* __restrict__ in, float4* __restrict__ out) {
  const long long e = (long long)blockIdx.x * LP_T + threadIdx.x;
  if (e >= total4) return;
  const int Ho = H / 2, Wo = W / 2;
  const int c = (int)(e % C4);
  const long long po = e / C4;
  const int xo = (int)(po % Wo);
  const long long r = po / Wo;
  const int yo = (int)(r % Ho);
  const long long img = r / Ho;
  const float4* s = in + ((size_t)(img * H + 2 * yo) * W + 2 * xo) * C4 + c;
  const float4 v0 = s[0], v1 = s[C4], v2 = s[(size_t)W * C4], v3 = s[(size_t)W * C4 + C4];
  float4 m;
  m.x = fmaxf(fmaxf(v0.x, v1.x), fmaxf(v2.x, v3.x));
  m.y = fmaxf(fmaxf(v0.y, v1.y), fmaxf(v2.y, v3.y));
  m.z = fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z));
  m.w = fmaxf(fmaxf(v0.w, v1.w), fmaxf(v2.w, v3.w));
  out[e] = m;
}

// ---------------------------------------------------------------------------------------------------- tap distance
__device__ __forceinline__ float lp_wave_sum(float v) {   // butterfly: every lane ends with the same bits
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// grid (ceil(HW / 256), N).  act: [2N][HW][C]; a wave per pixel, lanes over channels.  part[n * gridDim.x + chunk] = the chunk's sum
// of d = sum_c lin_c (xa_c / (|xa| + eps) - xb_c / (|xb| + eps))^2.
__global__ __launch_bounds__(LP_T) void k_lpips_tap(int N, int HW, int C, const float* __restrict__ act, const float* __restrict__ lin,
                                                    float* __restrict__ part) {
  __shared__ float red[LP_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.y;
  float w[LP_MAX_C / 64];
#pragma unroll
  for (int j = 0; j < LP_MAX_C / 64; ++j) w[j] = lane + 64 * j < C ? lin[lane + 64 * j] : 0.f;
  float wsum = 0.f;
  const int q0 = blockIdx.x * LP_TAP_PIX + wave * 64;
  for (int s = 0; s < 64; ++s) {
    const int q = q0 + s;
    if (q >= HW) break;   // the same for the whole wave
    const float* pa = act + ((size_t)n * HW + q) * C;
    const float* pb = act + ((size_t)(N + n) * HW + q) * C;
    float xa[LP_MAX_C / 64], xb[LP_MAX_C / 64];
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int j = 0; j < LP_MAX_C / 64; ++j) {
      const bool in = lane + 64 * j < C;
      xa[j] = in ? pa[lane + 64 * j] : 0.f;
      xb[j] = in ? pb[lane + 64 * j] : 0.f;
      sa = fmaf(xa[j], xa[j], sa);
      sb = fmaf(xb[j], xb[j], sb);
    }
    const float na = sqrtf(lp_wave_sum(sa)) + LP_EPS, nb = sqrtf(lp_wave_sum(sb)) + LP_EPS;
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < LP_MAX_C / 64; ++j) {
      const float diff = xa[j] / na - xb[j] / nb;
      d = fmaf(w[j] * diff, diff, d);
    }
    wsum += lp_wave_sum(d);
  }
  if (lane == 0) red[wave] = wsum;
  __syncthreads();
  if (tid == 0) part[(size_t)n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

struct LpFinish {
  int first[5];   // a tap's partial sums: part[first + n * count + i]
  int count[5];
  float hw[5];    // pixels of the tap
};

// grid (N), 5 waves: wave t finishes tap t, thread 0 the total
__global__ __launch_bounds__(320) void k_lpips_finish(LpFinish f, const float* __restrict__ part, float* __restrict__ lpips, float* __restrict__ taps) {
  __shared__ float tv[5];
  const int tid = threadIdx.x, lane = tid & 63, t = tid >> 6;
  const int n = blockIdx.x;
  const float* src = part + f.first[t] + (size_t)n * f.count[t];
  float s = 0.f;
  for (int i = lane; i < f.count[t]; i += 64) s += src[i];
  s = lp_wave_sum(s) / f.hw[t];
  if (lane == 0) {
    tv[t] = s;
    if (taps) taps[(size_t)n * 5 + t] = s;
  }
  __syncthreads();
  if (tid == 0) lpips[n] = (((tv[0] + tv[1]) + tv[2]) + tv[3]) + tv[4];
}

// ---------------------------------------------------------------------------------------------------- host side
constexpr int LP_CONVS[5] = {2, 2, 3, 3, 3};

struct LpPlan {
  bool ok = false;
  int h[5], w[5];
  size_t act_bytes = 0, part_bytes = 0;   // one activation buffer; all partial sums
  LpFinish fin;
  LpPlan(int N, int H, int W, const int* ch) {
    if (N <= 0 || N > 65535 || H < 16 || W < 16 || !ch) return;
    for (int b = 0; b < 5; ++b)
      if (ch[b] < 32 || ch[b] > LP_MAX_C || ch[b] % 32) return;
    long long elems = 0, parts = 0;
    for (int b = 0, hh = H, ww = W; b < 5; ++b, hh /= 2, ww /= 2) {
      h[b] = hh; w[b] = ww;
      const long long hw = (long long)hh * ww;
      if (hw > 0x7fffffffLL / 3) return;   // byte offsets inside a frame, and HW itself, are ints
      elems = std::max(elems, 2LL * N * hw * ch[b]);
      const long long chunks = (hw + LP_TAP_PIX - 1) / LP_TAP_PIX;
      fin.first[b] = (int)parts; fin.count[b] = (int)chunks; fin.hw[b] = (float)hw;
      parts += chunks * N;
      if (elems > 0x7fffffffLL || parts > 0x7fffffffLL) return;   // an activation buffer's element index fits an int
    }
    act_bytes = gs_align((size_t)elems * sizeof(float));
    part_bytes = gs_align((size_t)parts * sizeof(float));
    ok = true;
  }
};

int lp_conv(hipStream_t stream, int P, int H, int W, int Cin, int Cout, const float* in, const float* wt, const float* bias, float* out) {
  const int nt = Cout % 128 == 0 ? 4 : Cout % 96 == 0 ? 3 : Cout % 64 == 0 ? 2 : 1;
  const dim3 grid((unsigned)((P + MM_BM - 1) / MM_BM), (unsigned)(Cout / (32 * nt)));
  GS_KRANGE("lpips_conv");
  switch (nt) {
    case 4: hipLaunchKernelGGL(k_lpips_conv<4>, grid, dim3(MM_T), 0, stream, P, H, W, Cin, Cout, in, wt, bias, out); break;
    case 3: hipLaunchKernelGGL(k_lpips_conv<3>, grid, dim3(MM_T), 0, stream, P, H, W, Cin, Cout, in, wt, bias, out); break;
    case 2: hipLaunchKernelGGL(k_lpips_conv<2>, grid, dim3(MM_T), 0, stream, P, H, W, Cin, Cout, in, wt, bias, out); break;
    default: hipLaunchKernelGGL(k_lpips_conv<1>, grid, dim3(MM_T), 0, stream, P, H, W, Cin, Cout, in, wt, bias, out); break;
  }
  GS_CHECK_LAUNCH("lpips_conv");
  return MI355GS_OK;
}

}  // namespace

extern "C" {

size_t mi355gs_lpips_vgg_scratch_bytes(int N, int H, int W, const int channels[5]) {
  const LpPlan plan(N, H, W, channels);
  return plan.ok ? 2 * plan.act_bytes + plan.part_bytes : 0;
}

int mi355gs_lpips_vgg_rgb8(void* stream_, int N, int H, int W, const uint8_t* a, const uint8_t* b, const int channels[5],
                           const float* weights, void* scratch, float* lpips, float* taps) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const LpPlan plan(N, H, W, channels);
  if (!plan.ok || !a || !b || !weights || !scratch || !lpips) return MI355GS_EINVAL;
  if ((((uintptr_t)weights | (uintptr_t)scratch) & 15) != 0) return MI355GS_EINVAL;
  float* buf[2] = {(float*)scratch, (float*)((char*)scratch + plan.act_bytes)};
  float* part = (float*)((char*)scratch + 2 * plan.act_bytes);

  // the blob: per convolution [9 Cin][Cout] then [Cout]; then the five lin vectors
  const float* wp = weights;
  size_t conv_floats = 0;
  for (int blk = 0, cin = 3; blk < 5; ++blk)
    for (int l = 0; l < LP_CONVS[blk]; ++l, cin = channels[blk]) conv_floats += (size_t)9 * cin * channels[blk] + channels[blk];
  const float* lin = weights + conv_floats;

  int cur = 0, cin = 3;
  for (int blk = 0; blk < 5; ++blk) {
    const int C = channels[blk], h = plan.h[blk], w = plan.w[blk];
    const int P = 2 * N * h * w;
    if (blk > 0) {   // pool the previous block's tap into the other buffer
      const long long total4 = (long long)P * (cin / 4);
      GS_KRANGE("lpips_pool");
      hipLaunchKernelGGL(k_lpips_pool, dim3((unsigned)((total4 + LP_T - 1) / LP_T)), dim3(LP_T), 0, stream, total4, plan.h[blk - 1],
                         plan.w[blk - 1], cin / 4, (const float4*)buf[cur], (float4*)buf[cur ^ 1]);
      GS_CHECK_LAUNCH("lpips_pool");
      cur ^= 1;
    }
    for (int l = 0; l < LP_CONVS[blk]; ++l) {
      const float* wt = wp;
      const float* bias = wp + (size_t)9 * cin * C;
      wp = bias + C;
      if (blk == 0 && l == 0) {
        GS_KRANGE("lpips_conv0");
        hipLaunchKernelGGL(k_lpips_conv0, dim3((unsigned)((P + LP_P0 - 1) / LP_P0), (unsigned)(C / 32)), dim3(LP_T), 0, stream, N, H, W, C, a,
                           b, wt, bias, buf[cur]);
        GS_CHECK_LAUNCH("lpips_conv0");
      } else {
        const int rc = lp_conv(stream, P, h, w, cin, C, buf[cur], wt, bias, buf[cur ^ 1]);
        if (rc != MI355GS_OK) return rc;
        cur ^= 1;
      }
      cin = C;
    }
    GS_KRANGE("lpips_tap");
    hipLaunchKernelGGL(k_lpips_tap, dim3((unsigned)plan.fin.count[blk], (unsigned)N), dim3(LP_T), 0, stream, N, h * w, C, (const float*)buf[cur],
                       lin, part + plan.fin.first[blk]);
    GS_CHECK_LAUNCH("lpips_tap");
    lin += C;
  }
  GS_KRANGE("lpips_finish");
  hipLaunchKernelGGL(k_lpips_finish, dim3((unsigned)N), dim3(320), 0, stream, plan.fin, (const float*)part, lpips, taps);
  GS_CHECK_LAUNCH("lpips_finish");
  return MI355GS_OK;
}

}  // extern "C"
