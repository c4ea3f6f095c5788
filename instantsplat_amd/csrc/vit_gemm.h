// The row-major float32 GEMM of the transformer trunk (vit.hip) and of the dense heads (dpt.hip): the kernel template and its
// launcher, in one place as the matrix helper is in common.h.  Included inside each file's own translation unit.
#pragma once
#include "common.h"
#include <math.h>

namespace {

constexpr int VT_T = 256;
constexpr int VT_BM = 128;           // rows of a GEMM tile: 4 waves x 32
constexpr int VT_BK = 32;            // K chunk
constexpr int VT_LDA = VT_BK + 4;    // as lpips.hip: 16-byte aligned rows, rows 16 apart share a bank

enum { VT_PLAIN = 0, VT_GELU = 1, VT_RESID = 2 };

// ---------------------------------------------------------------------------------------------------- GEMM
// grid (ceil(M / 128), N / (32 NT)).  out[M][N] = epi(A[M][K] wt[K][N] + bias[N]); K a multiple of 32, N of 32 NT.
// VT_RESID: out = resid + (A wt + bias); resid may be out itself (every element is read and written by one thread).
template <int NT, int EPI>
__global__ __launch_bounds__(VT_T) void k_vit_gemm(int M, int K, int N, const float* __restrict__ A, const float* __restrict__ wt,
                                                   const float* __restrict__ bias, const float* resid, float* out) {
  constexpr int BN = 32 * NT;
  constexpr int LDB = BN + 32;   // rows k and k + 1 half the banks apart: the two lane halves do not collide
  __shared__ lp_f4 As4[VT_BM * VT_LDA / 4];
  __shared__ lp_f4 Bs4[VT_BK * LDB / 4];
  float* As = (float*)As4;
  float* Bs = (float*)Bs4;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile0 = blockIdx.x * VT_BM, n0 = blockIdx.y * BN;
  const int c4 = tid & 7;
  const int nq = K / VT_BK;
  lp_f4 ra[4], rb[NT];
  const lp_f4 zero4 = {0.f, 0.f, 0.f, 0.f};
  lp_acc16 acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  // round q stages chunk q - 1 from registers into LDS, fetches chunk q into registers (in flight under the matrix
  // instructions) and multiplies chunk q - 1
  for (int q = 0; q <= nq; ++q) {
    if (q > 0) {
      __syncthreads();   // the previous chunk has been consumed
#pragma unroll
      for (int i = 0; i < 4; ++i) *(lp_f4*)(As + ((tid >> 3) + 32 * i) * VT_LDA + 4 * c4) = ra[i];
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int f = tid + VT_T * j, row = f / (8 * NT), col4 = f - row * (8 * NT);
        *(lp_f4*)(Bs + row * LDB + 4 * col4) = rb[j];
      }
      __syncthreads();
    }
    if (q < nq) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = tile0 + (tid >> 3) + 32 * i;
        ra[i] = row < M ? *(const lp_f4*)(A + (size_t)row * K + q * VT_BK + 4 * c4) : zero4;
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int f = tid + VT_T * j, row = f / (8 * NT), col4 = f - row * (8 * NT);
        rb[j] = *(const lp_f4*)(wt + (size_t)(q * VT_BK + row) * N + n0 + 4 * col4);
      }
    }
    if (q > 0) {
#pragma unroll 4
      for (int kk = 0; kk < VT_BK / 2; ++kk)
#pragma unroll
        for (int j = 0; j < NT; ++j) lp_mfma_32x32x2(acc[j], As + 32 * wave * VT_LDA + 2 * kk, VT_LDA, Bs + 2 * kk * LDB + 32 * j, LDB, lane);
    }
  }

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
}

// Tile choice: 128 x 128 unless that leaves fewer workgroups than the 256 CUs, then 128 x 64 (M = 1728, N = 1024: 112 -> 224).
// THIN32 (dpt.hip only: the trunk's widths are multiples of 64, and vit.hip does not instantiate it): N a multiple of 32 but not
// of 64 runs 128 x 32 tiles.
template <bool THIN32 = false>
int vt_gemm(hipStream_t stream, int epi, int M, int K, int N, const float* A, const float* wt, const float* resid, float* out) {
  const int debug = 0;
  const float* bias = wt + (size_t)K * N;
  const unsigned mt = (unsigned)((M + VT_BM - 1) / VT_BM);
  const bool wide = N % 128 == 0 && (long long)mt * (N / 128) >= 256;
  const bool thin = THIN32 && N % 64 != 0;
  const dim3 grid(mt, (unsigned)(N / (wide ? 128 : thin ? 32 : 64)));
  GS_KRANGE("vit_gemm");
#define VT_LAUNCH(NT, EPI) hipLaunchKernelGGL((k_vit_gemm<NT, EPI>), grid, dim3(VT_T), 0, stream, M, K, N, A, wt, bias, resid, out)
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
