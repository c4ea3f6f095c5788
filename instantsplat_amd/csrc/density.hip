// Adaptive density control behind library calls (include/mi355gs.h, mi355gs_density_* / mi355gs_reset_opacity): what reference
// scene/gaussian_model.py:328-477 does with boolean indexing, `cat` and `zeros_like` over 6 parameter and 12 moment tensors —
// `add_densification_stats`, `densify_and_clone`, `densify_and_split`, `prune_points`, `densify_and_prune`, `reset_opacity` — as
// one ordered stream compaction with a little arithmetic on the appended rows.
//
//   statistics   1 dispatch  (k_density_stats)
//   plan         2 dispatches: the per-Gaussian decisions of one event + per-block class counts (k_density_plan), a one-workgroup
//                scan that loops over the block counts and leaves the totals on the device and in host memory (k_density_scan)
//   apply        1 dispatch: every input row read once, every output row written once (k_density_scatter)
//   reset        1 dispatch  (k_reset_opacity)
//
// No allocation, no memset, no host synchronisation, no atomics: every result is the same bits run to run.
// This file is compiled with -ffp-contract=off (Makefile): a decision must not depend on what a compiler chooses to fuse, and the
// statistics follow torch's operation order (square, add, correctly rounded sqrt).  Float division and sqrt are the correctly
// rounded ones (hipcc's default, -fhip-fp32-correctly-rounded-divide-sqrt).
#include "common.h"

namespace {

constexpr int DENSITY_BLOCK = 256;    // Gaussians per workgroup of the plan and scatter kernels: one per thread
constexpr int DENSITY_MAX_N = 8;      // children per split parent
constexpr int DENSITY_SCAN_THREADS = 1024;
// classes counted per block, in the order of the rows of `counts`
enum { CLS_ORIG = 0, CLS_CLONE = 1, CLS_SEL = 2, CLS_CLONE_SEL = 3, CLS_CHILD = 4 };   // CLS_CHILD + k: surviving children of copy k
constexpr int DENSITY_MAX_CLASSES = CLS_CHILD + DENSITY_MAX_N;
// bits of a Gaussian's code (mi355gs.h)
constexpr uint32_t CODE_ORIG = 1u, CODE_CLONE = 2u, CODE_SPLIT = 4u, CODE_CLONE_SEL = 8u;
constexpr int CODE_CHILD_SHIFT = 8;
// device totals (int32): what the scan leaves for the scatter and the host
enum { TOT_ORIG = 0, TOT_CLONE = 1, TOT_CHILD = 2, TOT_PRUNED = 3, TOT_SEL = 4, TOT_NEW_P = 5, TOT_CLONE_SEL = 6, TOT_CHILD_BASE = 8 };
constexpr int DENSITY_TOTALS = TOT_CHILD_BASE + DENSITY_MAX_N;   // 16 words

struct PlanArgs {
  int P, N, flags;
  const float *accum, *denom, *grads;
  int64_t n_grads;
  const uint8_t* mask;
  const float *max_radii, *scaling, *opacity;
  float max_grad, dense_limit, min_opacity, max_screen, world_limit, child_div;
};

__device__ __forceinline__ float density_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the reference's prune mask (scene/gaussian_model.py:467-471) of one row: opacity logit o, largest activated scale smax, radius
__device__ __forceinline__ bool density_pruned(const PlanArgs& a, float o, float smax, float radius) {
  bool p = density_sigmoid(o) < a.min_opacity;
  if (a.flags & MI355GS_DENSITY_SCREEN) p = p || radius > a.max_screen || smax > a.world_limit;
  return p;
}

// grid ceil(P / 256): code[i] and counts[class][block] — per wave and class one ballot and its popcount
__global__ __launch_bounds__(DENSITY_BLOCK) void k_density_plan(PlanArgs a, uint32_t* __restrict__ code, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_n[DENSITY_MAX_CLASSES][4];
  const int i = (int)blockIdx.x * DENSITY_BLOCK + (int)threadIdx.x;
  const bool densify = (a.flags & (MI355GS_DENSITY_CLONE | MI355GS_DENSITY_SPLIT)) != 0;
  uint32_t c = 0;
  if (i < a.P) {
    const float e0 = expf(a.scaling[3 * (size_t)i]), e1 = expf(a.scaling[3 * (size_t)i + 1]), e2 = expf(a.scaling[3 * (size_t)i + 2]);
    const float smax = fmaxf(fmaxf(e0, e1), e2);
    const float o = a.opacity[i];
    float g = 0.0f;
    if (densify) {
      if (a.grads) g = (int64_t)i < a.n_grads ? a.grads[i] : 0.0f;   // densify_and_split's padded gradient
      else {
        g = a.accum[i] / a.denom[i];
        if (g != g) g = 0.0f;   // grads[grads.isnan()] = 0.0
      }
    }
    // clone: ||grads|| >= max_grad (a one-column norm: |g|); split: the padded gradient itself.  The two size tests exclude each
    // other, and a clone's padded gradient is 0, so no Gaussian is both and no clone is split.
    const bool clone_sel = (a.flags & MI355GS_DENSITY_CLONE) && fabsf(g) >= a.max_grad && smax <= a.dense_limit;
    const bool split = (a.flags & MI355GS_DENSITY_SPLIT) && g >= a.max_grad && smax > a.dense_limit;
    // The reference's quirk: densification_postfix (:416-418) zeroes max_radii2D BEFORE densify_and_prune forms its mask, so
    // whenever clone / split ran the screen-size term sees zeros for every row; in the as-written prune-only form it sees the
    // real radii.
    bool pruned = false, child_pruned = false;
    if (a.flags & MI355GS_DENSITY_PRUNE) {
      if (a.mask) pruned = a.mask[i] != 0;
      else {   // the radii are read only where the screen-size term is asked for: without it max_radii may be null
        const float radius = ((a.flags & MI355GS_DENSITY_SCREEN) && !densify) ? a.max_radii[i] : 0.0f;
        pruned = density_pruned(a, o, smax, radius);
      }
      if (split && !a.mask) {
        // the children's scaling log(exp(s) / (0.8 N)), activated again as get_scaling does
        const float c0 = expf(logf(e0 / a.child_div)), c1 = expf(logf(e1 / a.child_div)), c2 = expf(logf(e2 / a.child_div));
        child_pruned = density_pruned(a, o, fmaxf(fmaxf(c0, c1), c2), 0.0f);
      }
    }
    if (!split && !pruned) c |= CODE_ORIG;          // split parents are always removed
    if (clone_sel) c |= CODE_CLONE_SEL;
    if (clone_sel && !pruned) c |= CODE_CLONE;      // a clone is its original's copy: the same mask value
    if (split) {
      c |= CODE_SPLIT;
      if (!child_pruned) c |= ((1u << a.N) - 1u) << CODE_CHILD_SHIFT;   // the N children share scaling and opacity
    }
    code[i] = c;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncls = CLS_CHILD + a.N;
  for (int k = 0; k < ncls; ++k) {
    const uint32_t bit = k < CLS_CHILD ? (k == CLS_ORIG ? CODE_ORIG : k == CLS_CLONE ? CODE_CLONE : k == CLS_SEL ? CODE_SPLIT : CODE_CLONE_SEL)
                                       : (1u << (CODE_CHILD_SHIFT + k - CLS_CHILD));
    const unsigned long long m = __ballot((c & bit) != 0);
    if (lane == 0) s_n[k][wave] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if ((int)threadIdx.x < ncls)
    counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (s_n[threadIdx.x][0] + s_n[threadIdx.x][1]) + (s_n[threadIdx.x][2] + s_n[threadIdx.x][3]);
}

// ONE workgroup: per class, counts[class][b] becomes the sum of counts[class][0 .. b), DENSITY_SCAN_THREADS block counts per turn of
// the loop with the running total carried from turn to turn — any number of blocks.  The totals go to totals_dev and, when given,
// to totals_host (words the device can write and the host can read: pinned, mapped host memory).
__global__ __launch_bounds__(DENSITY_SCAN_THREADS) void k_density_scan(int nblocks, int P, int N, uint32_t* counts,
                                                                       int32_t* __restrict__ totals_dev, int32_t* __restrict__ totals_host) {
  __shared__ uint32_t s_wave[DENSITY_SCAN_THREADS / 64];
  __shared__ uint32_t s_total[DENSITY_MAX_CLASSES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncls = CLS_CHILD + N;
  for (int k = 0; k < ncls; ++k) {
    uint32_t* cls = counts + (size_t)k * nblocks;
    uint32_t carry = 0;
    for (int first = 0; first < nblocks; first += DENSITY_SCAN_THREADS) {
      const int b = first + (int)threadIdx.x;
      const uint32_t v = b < nblocks ? cls[b] : 0u;
      uint32_t incl = v;
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      if (lane == 63) s_wave[wave] = incl;
      __syncthreads();
      uint32_t before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < DENSITY_SCAN_THREADS / 64; ++w) {
        const uint32_t t = s_wave[w];
        if (w < wave) before += t;
        total += t;
      }
      if (b < nblocks) cls[b] = carry + before + (incl - v);
      carry += total;
      __syncthreads();   // s_wave is rewritten by the next turn
    }
    if (threadIdx.x == 0) s_total[k] = carry;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t t[DENSITY_TOTALS];
    for (int k = 0; k < DENSITY_TOTALS; ++k) t[k] = 0;
    const int32_t n_orig = (int32_t)s_total[CLS_ORIG], n_clone = (int32_t)s_total[CLS_CLONE];
    int32_t base = n_orig + n_clone, n_child = 0;
    for (int k = 0; k < N; ++k) {   // .repeat(N, 1): copy 0 of every parent, then copy 1, ...
      t[TOT_CHILD_BASE + k] = base + n_child;
      n_child += (int32_t)s_total[CLS_CHILD + k];
    }
    t[TOT_ORIG] = n_orig; t[TOT_CLONE] = n_clone; t[TOT_CHILD] = n_child;
    t[TOT_SEL] = (int32_t)s_total[CLS_SEL]; t[TOT_CLONE_SEL] = (int32_t)s_total[CLS_CLONE_SEL];
    t[TOT_NEW_P] = base + n_child;
    // rows the reference's sequence built and removed again: (P + clones + N parents) - parents - new P
    t[TOT_PRUNED] = (P + t[TOT_CLONE_SEL] + (N - 1) * t[TOT_SEL]) - t[TOT_NEW_P];
    for (int k = 0; k < DENSITY_TOTALS; ++k) totals_dev[k] = t[k];
    if (totals_host)
      for (int k = 0; k < DENSITY_TOTALS; ++k) totals_host[k] = t[k];
  }
}

struct ScatterArgs {
  int P, N, rest_width, flags, nblocks;
  int32_t out_rows;       // rows the output tensors hold
  int64_t noise_rows;     // rows of `noise`
  const uint32_t* code;
  const uint32_t* offsets;   // the scanned counts
  const int32_t* totals;
  const float* noise;
  float child_div;
  const float* in[MI355GS_DENSITY_TENSORS];
  float* out[MI355GS_DENSITY_TENSORS];
};

constexpr int SCATTER_PARTS = 6;
constexpr int SLOTS = 2 + DENSITY_MAX_N;   // destinations of one input row: itself, its clone, its children
enum { MOVE_COPY = 0, MOVE_KEEP = 1, MOVE_ZERO = 2, MOVE_XYZ = 3, MOVE_SCALING = 4 };

// reference utils/general_utils.py build_rotation, one row of it: the quaternion is normalised with sqrt(w^2 + x^2 + y^2 + z^2)
__device__ __forceinline__ void density_rotation_row(const float* __restrict__ q4, int r, float R[3]) {
  const float norm = sqrtf(q4[0] * q4[0] + q4[1] * q4[1] + q4[2] * q4[2] + q4[3] * q4[3]);
  const float w = q4[0] / norm, x = q4[1] / norm, y = q4[2] / norm, z = q4[3] / norm;
  if (r == 0) { R[0] = 1.0f - 2.0f * (y * y + z * z); R[1] = 2.0f * (x * y - w * z); R[2] = 2.0f * (x * z + w * y); }
  else if (r == 1) { R[0] = 2.0f * (x * y + w * z); R[1] = 1.0f - 2.0f * (x * x + z * z); R[2] = 2.0f * (y * z - w * x); }
  else { R[0] = 2.0f * (x * z - w * y); R[1] = 2.0f * (y * z + w * x); R[2] = 1.0f - 2.0f * (x * x + y * y); }
}

// One element (row r of the block, column c, value v) of a tensor to every destination of its row.
template <int MODE>
__device__ __forceinline__ void density_emit(const ScatterArgs& a, float* __restrict__ out, int W, int r, int c, float v,
                                             const int32_t (*s_dst)[DENSITY_BLOCK], const int32_t* s_sel) {
  // s_dst[SLOTS][r]: the row's destinations as a bit mask, one bit per slot — most rows have one (themselves) or none
  for (uint32_t todo = (uint32_t)s_dst[SLOTS][r]; todo != 0; todo &= todo - 1) {
    const int s = __builtin_ctz(todo);
    const int32_t d = s_dst[s][r];
    float w = v;
    if (MODE == MOVE_ZERO || (MODE == MOVE_KEEP && s > 0)) w = 0.0f;   // every appended row starts with zero moments
    if ((MODE == MOVE_XYZ || MODE == MOVE_SCALING) && s >= 2) {
      const size_t i = (size_t)blockIdx.x * DENSITY_BLOCK + r;
      const float* sc = a.in[MI355GS_DENSITY_SCALING] + 3 * i;
      if (MODE == MOVE_SCALING) w = logf(expf(v) / a.child_div);   // scaling_inverse_activation(get_scaling / (0.8 N))
      else {
        // torch.normal(0, stds) = stds * z; bmm(R, sample) + xyz, the dot product summed in index order
        const int64_t zi = (int64_t)(s - 2) * a.totals[TOT_SEL] + s_sel[r];
        float z0 = 0.0f, z1 = 0.0f, z2 = 0.0f;
        if (a.noise && zi < a.noise_rows) { z0 = a.noise[3 * zi]; z1 = a.noise[3 * zi + 1]; z2 = a.noise[3 * zi + 2]; }
        float R[3];
        density_rotation_row(a.in[MI355GS_DENSITY_ROTATION] + 4 * i, c, R);
        const float s0 = expf(sc[0]) * z0, s1 = expf(sc[1]) * z1, s2 = expf(sc[2]) * z2;
        w = ((R[0] * s0 + R[1] * s1) + R[2] * s2) + v;
      }
    }
    out[(size_t)d * W + c] = w;
  }
}

// The block's `rows` rows of W floats: 16-byte loads over the block's span (it starts 16-byte aligned: 256 W floats per block),
// dword stores (a destination row of 3 or 45 floats is 4-byte aligned only); rows of 4 floats move as 16-byte stores too.
template <int WT, int MODE>
__device__ __forceinline__ void density_move(const ScatterArgs& a, int t, int w_rt, int rows, const int32_t (*s_dst)[DENSITY_BLOCK],
                                             const int32_t* s_sel) {
  const int W = WT ? WT : w_rt;
  float* __restrict__ out = a.out[t];
  if (!out || W == 0) return;
  if (MODE == MOVE_ZERO) {
    for (int e = threadIdx.x; e < rows * W; e += DENSITY_BLOCK) density_emit<MODE>(a, out, W, e / W, e % W, 0.0f, s_dst, s_sel);
    return;
  }
  const float* __restrict__ src = a.in[t] + (size_t)blockIdx.x * DENSITY_BLOCK * W;
  const int n = rows * W, nvec = n >> 2;
  if (WT == 4 && MODE == MOVE_COPY) {
    for (int r = threadIdx.x; r < rows; r += DENSITY_BLOCK) {
      const float4 v = ((const float4*)src)[r];
      for (uint32_t todo = (uint32_t)s_dst[SLOTS][r]; todo != 0; todo &= todo - 1) ((float4*)out)[s_dst[__builtin_ctz(todo)][r]] = v;
    }
    return;
  }
  for (int j = threadIdx.x; j < nvec; j += DENSITY_BLOCK) {
    const float4 v = ((const float4*)src)[j];
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int e = 4 * j + k;
      density_emit<MODE>(a, out, W, e / W, e % W, x[k], s_dst, s_sel);
    }
  }
  for (int e = 4 * nvec + (int)threadIdx.x; e < n; e += DENSITY_BLOCK) density_emit<MODE>(a, out, W, e / W, e % W, src[e], s_dst, s_sel);
}

template <int MODE>
__device__ __forceinline__ void density_move_rest(const ScatterArgs& a, int t, int rows, const int32_t (*s_dst)[DENSITY_BLOCK],
                                                  const int32_t* s_sel) {
  switch (a.rest_width) {   // 3 ((D + 1)^2 - 1) floats at max_sh_degree D
    case 0: return;
    case 9: density_move<9, MODE>(a, t, 0, rows, s_dst, s_sel); return;
    case 24: density_move<24, MODE>(a, t, 0, rows, s_dst, s_sel); return;
    case 45: density_move<45, MODE>(a, t, 0, rows, s_dst, s_sel); return;
    default: density_move<0, MODE>(a, t, a.rest_width, rows, s_dst, s_sel); return;
  }
}

// grid (ceil(P / 256), SCATTER_PARTS): block b's rows go where the scanned counts say.  Output order (the reference's): surviving
// originals in index order, surviving clones in index order, surviving children of copy 0 in index order, copy 1, ...
// blockIdx.y picks the tensors a workgroup moves — 0: the small parameter rows, the rates and the statistics, 1: f_rest, 2 / 3:
// the same split of exp_avg, 4 / 5: of exp_avg_sq — so that six times as many waves have loads in flight (one workgroup per 256
// rows leaves 3 waves per SIMD at 196,608 rows); each repeats the few ballots that place its rows.
__global__ __launch_bounds__(DENSITY_BLOCK) void k_density_scatter(ScatterArgs a) {
  const int part = (int)blockIdx.y;
  if ((part & 1) && a.rest_width == 0) return;   // no f_rest at max_sh_degree 0 (the whole workgroup leaves)
  __shared__ uint32_t s_seg[DENSITY_MAX_CLASSES][4];
  __shared__ int32_t s_dst[SLOTS + 1][DENSITY_BLOCK];   // [SLOTS]: which of a row's slots have a destination
  __shared__ int32_t s_sel[DENSITY_BLOCK];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = (int)blockIdx.x * DENSITY_BLOCK + (int)threadIdx.x;
  const uint32_t c = i < a.P ? a.code[i] : 0u;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int ncls = CLS_CHILD + a.N;
  uint32_t rank[DENSITY_MAX_CLASSES];
#pragma unroll
  for (int k = 0; k < DENSITY_MAX_CLASSES; ++k) {
    rank[k] = 0;
    if (k >= ncls) continue;
    const uint32_t bit = k < CLS_CHILD ? (k == CLS_ORIG ? CODE_ORIG : k == CLS_CLONE ? CODE_CLONE : k == CLS_SEL ? CODE_SPLIT : CODE_CLONE_SEL)
                                       : (1u << (CODE_CHILD_SHIFT + k - CLS_CHILD));
    const unsigned long long m = __ballot((c & bit) != 0);
    rank[k] = (uint32_t)__popcll(m & below);
    if (lane == 0) s_seg[k][wave] = (uint32_t)__popcll(m);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < DENSITY_MAX_CLASSES; ++k) {
    if (k >= ncls) continue;
    for (int w = 0; w < wave; ++w) rank[k] += s_seg[k][w];
    rank[k] += a.offsets[(size_t)k * a.nblocks + blockIdx.x];
  }
  {
    int64_t d0 = (c & CODE_ORIG) ? (int64_t)rank[CLS_ORIG] : -1;
    int64_t d1 = (c & CODE_CLONE) ? (int64_t)a.totals[TOT_ORIG] + rank[CLS_CLONE] : -1;
    if (d0 >= a.out_rows) d0 = -1;   // never past the caller's buffers
    if (d1 >= a.out_rows) d1 = -1;
    uint32_t have = (d0 >= 0 ? 1u : 0u) | (d1 >= 0 ? 2u : 0u);
    s_dst[0][threadIdx.x] = (int32_t)d0;
    s_dst[1][threadIdx.x] = (int32_t)d1;
#pragma unroll
    for (int k = 0; k < DENSITY_MAX_N; ++k) {
      if (k >= a.N) continue;
      int64_t d = (c >> (CODE_CHILD_SHIFT + k)) & 1u ? (int64_t)a.totals[TOT_CHILD_BASE + k] + rank[CLS_CHILD + k] : -1;
      if (d >= a.out_rows) d = -1;
      if (d >= 0) have |= 4u << k;
      s_dst[2 + k][threadIdx.x] = (int32_t)d;
    }
    s_dst[SLOTS][threadIdx.x] = (int32_t)have;
    s_sel[threadIdx.x] = (int32_t)rank[CLS_SEL];
  }
  __syncthreads();
  const int rows = min(DENSITY_BLOCK, a.P - (int)blockIdx.x * DENSITY_BLOCK);
  const int32_t (*dst)[DENSITY_BLOCK] = s_dst;
  if (part == 1) { density_move_rest<MOVE_COPY>(a, MI355GS_DENSITY_F_REST, rows, dst, s_sel); return; }
  if (part >= 2) {   // exp_avg (2, 3), exp_avg_sq (4, 5): survivors keep theirs, appended rows start at zero
    const int t0 = part < 4 ? MI355GS_DENSITY_EXP_AVG : MI355GS_DENSITY_EXP_AVG_SQ;
    if (part & 1) { density_move_rest<MOVE_KEEP>(a, t0 + MI355GS_DENSITY_F_REST, rows, dst, s_sel); return; }
    density_move<3, MOVE_KEEP>(a, t0 + MI355GS_DENSITY_XYZ, 0, rows, dst, s_sel);
    density_move<3, MOVE_KEEP>(a, t0 + MI355GS_DENSITY_F_DC, 0, rows, dst, s_sel);
    density_move<1, MOVE_KEEP>(a, t0 + MI355GS_DENSITY_OPACITY, 0, rows, dst, s_sel);
    density_move<3, MOVE_KEEP>(a, t0 + MI355GS_DENSITY_SCALING, 0, rows, dst, s_sel);
    density_move<4, MOVE_KEEP>(a, t0 + MI355GS_DENSITY_ROTATION, 0, rows, dst, s_sel);
    return;
  }
  density_move<3, MOVE_XYZ>(a, MI355GS_DENSITY_XYZ, 0, rows, dst, s_sel);
  density_move<3, MOVE_COPY>(a, MI355GS_DENSITY_F_DC, 0, rows, dst, s_sel);
  density_move<1, MOVE_COPY>(a, MI355GS_DENSITY_OPACITY, 0, rows, dst, s_sel);
  density_move<3, MOVE_SCALING>(a, MI355GS_DENSITY_SCALING, 0, rows, dst, s_sel);
  density_move<4, MOVE_COPY>(a, MI355GS_DENSITY_ROTATION, 0, rows, dst, s_sel);
  // the per-point learning-rate row: a survivor keeps it, a clone or child inherits its parent's (this project's rule: the
  // reference never resizes that tensor)
  density_move<1, MOVE_COPY>(a, MI355GS_DENSITY_PER_POINT_LR, 0, rows, dst, s_sel);
  // the statistics: zeroed whenever clone / split ran (densification_postfix), compacted in the prune-only form
  if (a.flags & (MI355GS_DENSITY_CLONE | MI355GS_DENSITY_SPLIT)) {
    density_move<1, MOVE_ZERO>(a, MI355GS_DENSITY_GRAD_ACCUM, 0, rows, dst, s_sel);
    density_move<1, MOVE_ZERO>(a, MI355GS_DENSITY_DENOM, 0, rows, dst, s_sel);
    density_move<1, MOVE_ZERO>(a, MI355GS_DENSITY_MAX_RADII, 0, rows, dst, s_sel);
  } else {
    density_move<1, MOVE_COPY>(a, MI355GS_DENSITY_GRAD_ACCUM, 0, rows, dst, s_sel);
    density_move<1, MOVE_COPY>(a, MI355GS_DENSITY_DENOM, 0, rows, dst, s_sel);
    density_move<1, MOVE_COPY>(a, MI355GS_DENSITY_MAX_RADII, 0, rows, dst, s_sel);
  }
}

// add_densification_stats (:476-478) and train.py:198 for the rows with filter != 0 (filter null: radii > 0)
__global__ __launch_bounds__(256) void k_density_stats(int P, const float* __restrict__ grad, int grad_stride, const uint8_t* __restrict__ filter,
                                                       const int32_t* __restrict__ radii, float* __restrict__ accum, float* __restrict__ denom,
                                                       float* __restrict__ max_radii) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= P) return;
  if (!(filter ? filter[i] != 0 : radii[i] > 0)) return;
  const float gx = grad[(size_t)i * grad_stride], gy = grad[(size_t)i * grad_stride + 1];
  accum[i] += sqrtf(gx * gx + gy * gy);
  denom[i] += 1.0f;
  if (radii && max_radii) max_radii[i] = fmaxf(max_radii[i], (float)radii[i]);
}

// reset_opacity (:280-283): inverse_sigmoid(min(sigmoid(o), 0.01)); replace_tensor_to_optimizer zeroes both moments
__global__ __launch_bounds__(256) void k_reset_opacity(int P, float* __restrict__ opacity, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq) {
  const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= P) return;
  const float x = fminf(density_sigmoid(opacity[i]), 0.01f);
  opacity[i] = logf(x / (1.0f - x));
  if (exp_avg) exp_avg[i] = 0.0f;
  if (exp_avg_sq) exp_avg_sq[i] = 0.0f;
}

// new P <= (N + 1) P must stay an int
bool density_size_ok(int P, int N) { return P > 0 && N >= 1 && N <= DENSITY_MAX_N && (long long)P * (N + 1) <= 0x7fffffffLL; }
int density_blocks(int P) { return (P + DENSITY_BLOCK - 1) / DENSITY_BLOCK; }
size_t density_counts_bytes(int P) { return gs_align((size_t)DENSITY_MAX_CLASSES * density_blocks(P) * sizeof(uint32_t)); }

}  // namespace

extern "C" {

int mi355gs_density_stats(void* stream_, int P, const float* grad, int grad_stride, const uint8_t* filter, const int32_t* radii,
                          float* grad_accum, float* denom, float* max_radii) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (P <= 0 || !grad || grad_stride < 2 || (!filter && !radii) || !grad_accum || !denom) return MI355GS_EINVAL;
  GS_KRANGE("density_stats");
  hipLaunchKernelGGL(k_density_stats, dim3((P + 255) / 256), dim3(256), 0, stream, P, grad, grad_stride, filter, radii, grad_accum, denom, max_radii);
  GS_CHECK_LAUNCH("density_stats");
  return MI355GS_OK;
}

size_t mi355gs_density_scratch_bytes(int P, int N) {
  if (!density_size_ok(P, N)) return 0;
  return density_counts_bytes(P) + gs_align(DENSITY_TOTALS * sizeof(int32_t));
}

int mi355gs_density_plan(void* stream_, int P, int N, int flags, const float* grad_accum, const float* denom, const float* grads,
                         int64_t n_grads, const uint8_t* mask, const float* max_radii, const float* scaling, const float* opacity,
                         float max_grad, float dense_limit, float min_opacity, float max_screen_size, float world_limit,
                         float child_div, uint32_t* code, void* scratch, int32_t* totals_host) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const int all = MI355GS_DENSITY_CLONE | MI355GS_DENSITY_SPLIT | MI355GS_DENSITY_PRUNE | MI355GS_DENSITY_SCREEN;
  if (!density_size_ok(P, N) || (flags & ~all) || !(flags & (all & ~MI355GS_DENSITY_SCREEN)) || !scaling || !opacity || !code || !scratch)
    return MI355GS_EINVAL;
  const bool densify = (flags & (MI355GS_DENSITY_CLONE | MI355GS_DENSITY_SPLIT)) != 0;
  if (densify && !grads && (!grad_accum || !denom)) return MI355GS_EINVAL;
  if (grads && n_grads < 0) return MI355GS_EINVAL;
  if ((flags & MI355GS_DENSITY_SCREEN) && !(flags & MI355GS_DENSITY_PRUNE)) return MI355GS_EINVAL;
  if ((flags & MI355GS_DENSITY_PRUNE) && !mask && (flags & MI355GS_DENSITY_SCREEN) && !densify && !max_radii) return MI355GS_EINVAL;
  if ((flags & MI355GS_DENSITY_SPLIT) && !(child_div > 0.0f)) return MI355GS_EINVAL;
  const int nblocks = density_blocks(P);
  uint32_t* counts = (uint32_t*)scratch;
  int32_t* totals = (int32_t*)((char*)scratch + density_counts_bytes(P));
  PlanArgs a{P, N, flags, grad_accum, denom, grads, n_grads, mask, max_radii, scaling, opacity,
             max_grad, dense_limit, min_opacity, max_screen_size, world_limit, child_div};
  GS_KRANGE("density_plan");
  hipLaunchKernelGGL(k_density_plan, dim3(nblocks), dim3(DENSITY_BLOCK), 0, stream, a, code, counts);
  GS_CHECK_LAUNCH("density_plan");
  GS_KRANGE("density_scan");
  hipLaunchKernelGGL(k_density_scan, dim3(1), dim3(DENSITY_SCAN_THREADS), 0, stream, nblocks, P, N, counts, totals, totals_host);
  GS_CHECK_LAUNCH("density_scan");
  return MI355GS_OK;
}

int mi355gs_density_apply(void* stream_, int P, int N, int flags, int rest_width, const uint32_t* code, const void* scratch,
                          const float* noise, int64_t noise_rows, int64_t n_selected, float child_div, const void* const* in,
                          void* const* out, int64_t out_rows) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!density_size_ok(P, N) || rest_width < 0 || rest_width > 3 * 255 || !code || !scratch || !in || !out) return MI355GS_EINVAL;
  if (out_rows < 0 || out_rows > 0x7fffffffLL || noise_rows < 0 || n_selected < 0 || n_selected > P) return MI355GS_EINVAL;
  if ((flags & MI355GS_DENSITY_SPLIT) && n_selected > 0 && (!noise || noise_rows < (int64_t)N * n_selected || !(child_div > 0.0f)))
    return MI355GS_EINVAL;   // something is split: every child needs its normal sample
  if (out_rows == 0) return MI355GS_OK;   // everything was pruned: nothing to write
  ScatterArgs a;
  a.P = P; a.N = N; a.rest_width = rest_width; a.flags = flags; a.nblocks = density_blocks(P);
  a.out_rows = (int32_t)out_rows; a.noise_rows = noise_rows; a.code = code; a.offsets = (const uint32_t*)scratch;
  a.totals = (const int32_t*)((const char*)scratch + density_counts_bytes(P));
  a.noise = noise; a.child_div = child_div;
  for (int t = 0; t < MI355GS_DENSITY_TENSORS; ++t) {
    a.in[t] = (const float*)in[t];
    a.out[t] = (float*)out[t];
    const bool param = t < MI355GS_DENSITY_EXP_AVG && !(t == MI355GS_DENSITY_F_REST && rest_width == 0);
    if (param && (!in[t] || !out[t])) return MI355GS_EINVAL;   // the parameters are required; moments, rates and statistics
    if (out[t] && !in[t]) return MI355GS_EINVAL;               // move only where both sides are given
    if (!in[t]) a.out[t] = nullptr;
  }
  if ((uintptr_t)a.out[MI355GS_DENSITY_ROTATION] & 15) return MI355GS_EINVAL;   // rows of four floats move as 16 bytes
  for (int t = 0; t < MI355GS_DENSITY_TENSORS; ++t)
    if ((uintptr_t)a.in[t] & 15) return MI355GS_EINVAL;   // the 16-byte loads over a block's span
  GS_KRANGE("density_scatter");
  hipLaunchKernelGGL(k_density_scatter, dim3(a.nblocks, SCATTER_PARTS), dim3(DENSITY_BLOCK), 0, stream, a);
  GS_CHECK_LAUNCH("density_scatter");
  return MI355GS_OK;
}

int mi355gs_reset_opacity(void* stream_, int P, float* opacity, float* exp_avg, float* exp_avg_sq) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (P <= 0 || !opacity) return MI355GS_EINVAL;
  GS_KRANGE("reset_opacity");
  hipLaunchKernelGGL(k_reset_opacity, dim3((P + 255) / 256), dim3(256), 0, stream, P, opacity, exp_avg, exp_avg_sq);
  GS_CHECK_LAUNCH("reset_opacity");
  return MI355GS_OK;
}

}  // extern "C"
