// The float32 matrix-instruction tile of LPIPS (lpips.hip), the transformer trunk (vit.hip) and the dense heads (dpt.hip): the tile
// constants, the ONE software-pipelined K loop, the 3 x 3 tap fetch of the implicit-GEMM convolutions, and the row-major GEMM with
// its launcher.  A kernel is its LDS declarations, a fetch and an epilogue.  Included in each file's own unit.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int MM_T = 256;            // threads: 4 waves
constexpr int MM_BM = 128;           // rows (GEMM) or pixels (convolution) of a tile: 4 waves x 32
constexpr int MM_BK = 32;            // K chunk; a convolution's is 32 channels of one tap
constexpr int MM_LDA = MM_BK + 4;    // LDS row of the A tile: 16-byte aligned rows, rows 16 apart share a bank (2-way)
// LDS row of the B tile (32 NT columns): + 32 puts rows k and k + 1 half the banks apart, so the two lane halves do not collide.
// The GEMM always pads; the convolutions only where 32 NT is a multiple of 64 (their NT 1 and 3 tiles keep 22528 and 30720 bytes).
constexpr int mm_ldb(int NT, bool gemm) { return 32 * NT + ((gemm || NT % 2 == 0) ? 32 : 0); }

// ---------------------------------------------------------------------------------------------------- the K loop
// acc[j] = sum over nq chunks of A (x) wt for columns n0 + 32 j + (0..31) of the tile's 128 rows, then epilogue(acc).  wt is
// [32 nq][N] row-major.  A thread stages four items of A per chunk and NT of the weights.  fetch(q, i) RETURNS item i of A's
// chunk q: floats 4 (tid & 7) .. + 3 of tile row (tid >> 3) + 32 i, zeros where there is nothing to read.  Round q stages chunk
// q - 1 from registers into LDS, fetches chunk q into registers (in flight under the matrix instructions) and multiplies chunk
// q - 1: two barriers per chunk.
// Nothing the loop holds in registers crosses a call by reference, on purpose.  The accumulators are LOCAL to
// this function: handed in from the kernel they cost 50 more VGPRs at NT = 4 (130 + 64 AGPR, 2 waves per SIMD instead of 79 + 64
// and 3).  The fetch returns its item by value and captures by value: filling `ra` through a reference, or a fetch lambda that
// captures the kernel's locals by reference, compiles to the same registers but a later-scheduled LDS address in the multiply
// block, 3 to 7 % of the kernel's time.
template <int NT, int LDB, class Fetch, class Epilogue>
__device__ __forceinline__ void mm_k_loop(int nq, const float* __restrict__ wt, int N, int n0, float* As, float* Bs, Fetch fetch,
                                          Epilogue epilogue) {
  lp_acc16 acc[NT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c4 = tid & 7;
  lp_f4 ra[4], rb[NT];
  int brow[NT], bcol[NT];   // weight item j of the chunk's 32 x 32 NT floats: the float4 at column bcol[j] of row brow[j]
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int f = tid + MM_T * j;
    brow[j] = f / (8 * NT);
    bcol[j] = 4 * (f - brow[j] * (8 * NT));
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  }

  for (int q = 0; q <= nq; ++q) {
    if (q > 0) {
      __syncthreads();   // the previous chunk has been consumed
#pragma unroll
      for (int i = 0; i < 4; ++i) *(lp_f4*)(As + ((tid >> 3) + 32 * i) * MM_LDA + 4 * c4) = ra[i];
#pragma unroll
      for (int j = 0; j < NT; ++j) *(lp_f4*)(Bs + brow[j] * LDB + bcol[j]) = rb[j];
      __syncthreads();
    }
    if (q < nq) {
#pragma unroll
      for (int i = 0; i < 4; ++i) ra[i] = fetch(q, i);
#pragma unroll
      for (int j = 0; j < NT; ++j) rb[j] = *(const lp_f4*)(wt + (size_t)(q * MM_BK + brow[j]) * N + n0 + bcol[j]);
    }
    if (q > 0) {
#pragma unroll 4
      for (int kk = 0; kk < MM_BK / 2; ++kk)
#pragma unroll
        for (int j = 0; j < NT; ++j) lp_mfma_32x32x2(acc[j], As + 32 * wave * MM_LDA + 2 * kk, MM_LDA, Bs + 2 * kk * LDB + 32 * j, LDB, lane);
    }
  }
  epilogue(acc);
}

// ---------------------------------------------------------------------------------------------------- 3 x 3 tap fetch
struct MmConv {
  int P;                 // output pixels of the call: images x Ho x Wo
  int Hi, Wi, Ho, Wo;    // Ho = ceil(Hi / stride)
  int Cin, Cout, stride, relu_in;
};

// The A side of a 3 x 3, padding 1 convolution as an implicit GEMM over in [image][Hi][Wi][Cin] (Cin a multiple of 32): a row is
// an output pixel, k = (3 ky + kx) Cin + ci, so chunk q is 32 channels of ONE tap and wt is a plain [9 Cin][Cout] matrix.
// Border taps (and rows past P) are predicated loads that yield zero: nothing outside the buffer is read.  relu_in: ReLU on
// the staged input.  UNIT: stride 1 and no ReLU on the way in, known at compile time: output pixel p sits on input pixel p, four
// indices in one register, which keeps the NT = 1 tiles at 7 waves per SIMD.  g.stride and g.relu_in are NOT
// read then: a UNIT caller's geometry must have stride 1, relu_in 0, Ho = Hi and Wo = Wi (both callers build it so).
template <bool UNIT>
struct MmTapFetch {
  const MmConv& g;
  const float* __restrict__ in;
  int cchunks, nq, base[4], iy[4], ix[4];   // chunks per tap and in all; the thread's four pixels: index, row, column in the input
  __device__ __forceinline__ MmTapFetch(const MmConv& g_, const float* __restrict__ in_) : g(g_), in(in_), cchunks(g_.Cin / MM_BK), nq(9 * cchunks) {
    const int HWo = g.Ho * g.Wo;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = blockIdx.x * MM_BM + (threadIdx.x >> 3) + 32 * i;
      iy[i] = -2;   // a row past P: every tap of it fails the row test
      ix[i] = base[i] = 0;
      if (p < g.P) {
        const int e = p / HWo, rem = p - e * HWo, oy = rem / g.Wo, ox = rem - oy * g.Wo;
        iy[i] = UNIT ? oy : oy * g.stride;
        ix[i] = UNIT ? ox : ox * g.stride;
        base[i] = UNIT ? p : (e * g.Hi + iy[i]) * g.Wi + ix[i];
      }
    }
  }
  __device__ __forceinline__ lp_f4 operator()(int q, int i) const {
    const int t = q / cchunks, c0 = (q - t * cchunks) * MM_BK;
    const int dy = t / 3 - 1, dx = t % 3 - 1;
    const bool ok = (unsigned)(iy[i] + dy) < (unsigned)g.Hi && (unsigned)(ix[i] + dx) < (unsigned)g.Wi;
    lp_f4 v = ok ? *(const lp_f4*)(in + (size_t)(base[i] + dy * g.Wi + dx) * g.Cin + c0 + 4 * (threadIdx.x & 7)) : lp_f4{0.f, 0.f, 0.f, 0.f};
    const bool relu = !UNIT && g.relu_in;   // a select per element, not a branch round the four: k_dpt_conv<1> keeps 7 waves
#pragma unroll
    for (int k = 0; k < 4; ++k) LP_AT(v, k) = relu ? fmaxf(LP_AT(v, k), 0.f) : LP_AT(v, k);
    return v;
  }
};

// ---------------------------------------------------------------------------------------------------- GEMM
enum { VT_PLAIN = 0, VT_GELU = 1, VT_RESID = 2 };

// grid (ceil(M / 128), N / (32 NT)).  out[M][N] = epi(A[M][K] wt[K][N] + bias[N]); K a multiple of 32, N of 32 NT.
// VT_RESID: out = resid + (A wt + bias); resid may be out itself (every element is read and written by one thread).
template <int NT, int EPI>
__global__ __launch_bounds__(MM_T) void k_vit_gemm(int M, int K, int N, const float* __restrict__ A, const float* __restrict__ wt,
                                                   const float* __restrict__ bias, const float* resid, float* out) {
  constexpr int LDB = mm_ldb(NT, true);
  __shared__ lp_f4 As4[MM_BM * MM_LDA / 4];
  __shared__ lp_f4 Bs4[MM_BK * LDB / 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile0 = blockIdx.x * MM_BM, n0 = blockIdx.y * 32 * NT;
  const auto fetch = [=](int q, int i) {
    const int row = tile0 + (tid >> 3) + 32 * i;
    return row < M ? *(const lp_f4*)(A + (size_t)row * K + q * MM_BK + 4 * (tid & 7)) : lp_f4{0.f, 0.f, 0.f, 0.f};
  };
  mm_k_loop<NT, LDB>(K / MM_BK, wt, N, n0, (float*)As4, (float*)Bs4, fetch, [&](lp_acc16 (&acc)[NT]) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int n = n0 + 32 * j + (lane & 31);
      const float bv = bias[n];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = tile0 + 32 * wave + lp_acc_row(r, lane);
        if (row < M) {
          const size_t o = (size_t)row * N + n;
          float y = acc[j][r] + bv;
          if (EPI == VT_GELU) y = 0.5f * y * (1.0f + erff(y * 0.70710678118654752440f));
          if (EPI == VT_RESID) y = resid[o] + y;
          out[o] = y;
        }
      }
    }
  });
}

// Tile choice: 128 x 128 unless that leaves fewer workgroups than the 256 CUs, then 128 x 64 (M = 1728, N = 1024: 112 -> 224).
// THIN32 (dpt.hip only: the trunk's widths are multiples of 64, and vit.hip does not instantiate it): N a multiple of 32 but not
// of 64 runs 128 x 32 tiles.
template <bool THIN32 = false>
int vt_gemm(hipStream_t stream, int epi, int M, int K, int N, const float* A, const float* wt, const float* resid, float* out) {
  const float* bias = wt + (size_t)K * N;
  const unsigned mt = (unsigned)((M + MM_BM - 1) / MM_BM);
  const bool wide = N % 128 == 0 && (long long)mt * (N / 128) >= 256;
  const bool thin = THIN32 && N % 64 != 0;
  const dim3 grid(mt, (unsigned)(N / (wide ? 128 : thin ? 32 : 64)));
  GS_KRANGE("vit_gemm");
#define VT_LAUNCH(NT, EPI) hipLaunchKernelGGL((k_vit_gemm<NT, EPI>), grid, dim3(MM_T), 0, stream, M, K, N, A, wt, bias, resid, out)
  if (wide) {
    if (epi == VT_PLAIN) VT_LAUNCH(4, VT_PLAIN); else if (epi == VT_GELU) VT_LAUNCH(4, VT_GELU); else VT_LAUNCH(4, VT_RESID);
  } else if (!thin) {
    if (epi == VT_PLAIN) VT_LAUNCH(2, VT_PLAIN); else if (epi == VT_GELU) VT_LAUNCH(2, VT_GELU); else VT_LAUNCH(2, VT_RESID);
  } else if constexpr (THIN32) {
    if (epi == VT_PLAIN) VT_LAUNCH(1, VT_PLAIN); else if (epi == VT_GELU) VT_LAUNCH(1, VT_GELU); else VT_LAUNCH(1, VT_RESID);
  }
#undef VT_LAUNCH
  GS_CHECK_LAUNCH("vit_gemm");
  return MI355GS_OK;
}

}  // namespace
