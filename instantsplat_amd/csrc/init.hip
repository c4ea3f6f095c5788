// The tail of the init stage behind library calls (include/mi355gs.h, mi355gs_pointmap_stats / mi355gs_covis_masks /
// mi355gs_compact_pointmaps): what reference init_geo.py:61-129 does between the aligner's pointmaps and the directory train.py
// opens — confidence-aware ranking, co-visibility masks (utils/sfm_utils.py:342-432, `compute_co_vis_masks`) and the boolean
// compaction of points, colours and confidences (`save_points3D`, :264-277).
//
//   statistics   2 dispatches: one pass over the V depth maps and confidences (per-workgroup min / max / confidence sum, and the
//                overlap mask cleared on the way: no memset), one finishing launch per view in a fixed order
//   masks        1 dispatch over all V (V - 1) / 2 ordered pairs (target of rank i, source of rank j < i)
//   compaction   3 dispatches: keep-count per block of COMPACT_BLOCK elements, a one-workgroup scan that loops over the block
//                counts (any number of them), the ordered scatter
//
// No allocation, no memset, no host synchronisation, no atomics: every result is the same bits run to run.
// This file is compiled with -ffp-contract=off (Makefile): the masks must equal the reference's numpy arithmetic pixel for
// pixel, so every product and sum below is rounded where the source says.  Float division is the correctly rounded one (hipcc's
// default, -fhip-fp32-correctly-rounded-divide-sqrt).
#include "common.h"

namespace {

constexpr int STATS_PER_THREAD = 16;
constexpr int STATS_CHUNK = 256 * STATS_PER_THREAD;   // elements of one view per workgroup of the statistics pass
constexpr int COMPACT_ROUNDS = 4;
constexpr int COMPACT_BLOCK = 256 * COMPACT_ROUNDS;   // elements per workgroup of the count and scatter kernels
constexpr int SCAN_THREADS = 1024;
constexpr int MAX_VIEWS = 256;

struct StatsPartial { double sum; float mn, mx; };
struct ViewOrder { uint8_t v[MAX_VIEWS]; };   // the ranking, by value in the kernel arguments (V <= 256)

// numpy's min / max propagate a NaN; so do these, whatever the order of the combination
__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// -> (min, max) over the workgroup's 256 threads, in every thread
__device__ __forceinline__ void block_min_max(float& mn, float& mx, float* lds /* [8] */) {
  for (int m = 32; m >= 1; m >>= 1) {
    mn = nan_min(mn, __shfl_xor(mn, m));
    mx = nan_max(mx, __shfl_xor(mx, m));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { lds[wave] = mn; lds[4 + wave] = mx; }
  __syncthreads();
  mn = nan_min(nan_min(lds[0], lds[1]), nan_min(lds[2], lds[3]));
  mx = nan_max(nan_max(lds[4], lds[5]), nan_max(lds[6], lds[7]));
}

// grid (chunks, V): min / max of the depths and the double sum of the confidences of STATS_CHUNK elements of one view; the
// view's bytes of the overlap mask are cleared by the threads that read its depths.
__global__ __launch_bounds__(256) void k_pointmap_stats(int HW, const float* __restrict__ depth, const float* __restrict__ conf,
                                                        uint8_t* __restrict__ overlap, StatsPartial* __restrict__ part) {
  __shared__ float s_mm[8];
  __shared__ double s_sum[4];
  const size_t view = (size_t)blockIdx.y * (size_t)HW;
  const int first = (int)blockIdx.x * STATS_CHUNK + (int)threadIdx.x;   // < HW + 256: HW <= 2^31 - 1 - STATS_CHUNK
  float mn = depth[view + min(first, HW - 1)], mx = mn;   // an element of the view for the threads past its end
  double sum = 0.0;
#pragma unroll 4
  for (int k = 0; k < STATS_PER_THREAD; ++k) {
    const int e = first + k * 256;
    if (e < HW) {
      const float d = depth[view + e];
      mn = nan_min(mn, d);
      mx = nan_max(mx, d);
      sum += (double)conf[view + e];
      overlap[view + e] = 0;
    }
  }
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  block_min_max(mn, mx, s_mm);   // (its barrier also orders s_sum)
  if (threadIdx.x == 0) {
    StatsPartial p;
    p.sum = (s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3]);
    p.mn = mn; p.mx = mx;
    part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
  }
}

// grid V: stats[v] = (min, max, confidence sum) as doubles, the partials combined in a fixed order
__global__ __launch_bounds__(256) void k_pointmap_stats_finish(int chunks, const StatsPartial* __restrict__ part, double* __restrict__ stats) {
  __shared__ float s_mm[8];
  __shared__ double s_sum[256];
  const StatsPartial* __restrict__ p = part + (size_t)blockIdx.x * chunks;
  float mn = p[0].mn, mx = p[0].mx;
  double sum = 0.0;
  for (int k = threadIdx.x; k < chunks; k += 256) {
    mn = nan_min(mn, p[k].mn);
    mx = nan_max(mx, p[k].mx);
    sum += p[k].sum;
  }
  s_sum[threadIdx.x] = sum;
  block_min_max(mn, mx, s_mm);
  for (int m = 128; m >= 1; m >>= 1) {
    if ((int)threadIdx.x < m) s_sum[threadIdx.x] += s_sum[threadIdx.x + m];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    stats[3 * blockIdx.x] = (double)mn;
    stats[3 * blockIdx.x + 1] = (double)mx;
    stats[3 * blockIdx.x + 2] = s_sum[0];
  }
}

// grid (ceil(HW / 256), V (V - 1) / 2): pair p = i (i - 1) / 2 + j is target view c = order[i], source view s = order[j], j < i.
// reference utils/sfm_utils.py:342-432 for one point of s, quirks included:
//   project_points: float32 inputs widened to double (its hstack with a float64 column), cam = E [p,1], h = K cam, (x, y) = h / h2;
//   the bounds test on the doubles (a point behind the camera that lands inside the frame passes; h2 = 0 gives inf / NaN, which fail);
//   the pixel is the truncation; the compared depth is the point's depth in ITS OWN view, normalised in float32 with the min / max
//   over all views ranked before c, against c's depth map at the pixel normalised with c's own min / max; a constant map gives
//   0 / 0 = NaN and no hit.  A hit is a plain byte store of 1: many threads may store the same value.
__global__ __launch_bounds__(256) void k_covis_masks(int W, int H, ViewOrder order, const float* __restrict__ points,
                                                     const float* __restrict__ depth, const float* __restrict__ K,
                                                     const float* __restrict__ w2c, const double* __restrict__ stats, float threshold,
                                                     uint8_t* __restrict__ overlap) {
  __shared__ float s_mm[8];
  const int p = (int)blockIdx.y;   // <= 32639: exact in float
  int i = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
  while (i * (i - 1) / 2 > p) --i;
  while ((i + 1) * i / 2 <= p) ++i;
  const int j = p - i * (i - 1) / 2;
  const int c = order.v[i], s = order.v[j];
  // min / max over the union of the views ranked before c: thread t < i brings view order[t] (i <= 255)
  const int mine = order.v[min((int)threadIdx.x, i - 1)];
  float bmin = (float)stats[3 * mine], bmax = (float)stats[3 * mine + 1];
  block_min_max(bmin, bmax, s_mm);
  const float cmin = (float)stats[3 * c], cmax = (float)stats[3 * c + 1];
  const int HW = W * H;
  const int e = (int)(blockIdx.x * 256u + threadIdx.x);
  if (e >= HW) return;
  const size_t src = (size_t)s * (size_t)HW + (size_t)e;
  const double px = (double)points[3 * src], py = (double)points[3 * src + 1], pz = (double)points[3 * src + 2];
  const float* __restrict__ E = w2c + 16 * c;
  const float* __restrict__ Kc = K + 9 * c;
  double cam[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    cam[r] = (((double)E[4 * r] * px + (double)E[4 * r + 1] * py) + (double)E[4 * r + 2] * pz) + (double)E[4 * r + 3];
  double h[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) h[r] = ((double)Kc[3 * r] * cam[0] + (double)Kc[3 * r + 1] * cam[1]) + (double)Kc[3 * r + 2] * cam[2];
  const double x = h[0] / h[2], y = h[1] / h[2];
  if (!(x >= 0.0 && x < (double)W && y >= 0.0 && y < (double)H)) return;
  const int xi = (int)x, yi = (int)y;   // in [0, W) x [0, H) by the test above
  const size_t dst = (size_t)c * (size_t)HW + (size_t)yi * (size_t)W + (size_t)xi;
  const float a = (depth[src] - bmin) / (bmax - bmin);
  const float b = (depth[dst] - cmin) / (cmax - cmin);
  if (fabsf(a - b) < threshold) overlap[dst] = 1;
}

// element e is kept when it lies inside the arrays and its overlap byte is 0 (no mask: everything is kept)
__device__ __forceinline__ bool compact_keep(int64_t e, int64_t n, const uint8_t* __restrict__ overlap) {
  return e < n && (!overlap || overlap[e] == 0);
}

// grid ceil(n / COMPACT_BLOCK): counts[b] = kept elements of block b — per wave and round one ballot and its popcount
__global__ __launch_bounds__(256) void k_compact_count(int64_t n, const uint8_t* __restrict__ overlap, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_n[4];
  const int64_t base = (int64_t)blockIdx.x * COMPACT_BLOCK + threadIdx.x;
  uint32_t kept = 0;
#pragma unroll
  for (int r = 0; r < COMPACT_ROUNDS; ++r) kept += (uint32_t)__popcll(__ballot(compact_keep(base + r * 256, n, overlap)));
  if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = (s_n[0] + s_n[1]) + (s_n[2] + s_n[3]);
}

// ONE workgroup: offsets[b] = sum of counts[0 .. b), SCAN_THREADS block counts per turn of the loop with the running total
// carried from turn to turn — any number of blocks.  The total goes to *count_dev and, when given, to *count_host (a word the
// device can write and the host can read: pinned, mapped host memory).  counts and offsets may be the same array.
__global__ __launch_bounds__(SCAN_THREADS) void k_compact_scan(int nblocks, const uint32_t* counts, uint32_t* offsets,
                                                               int32_t* __restrict__ count_dev, int32_t* __restrict__ count_host) {
  __shared__ uint32_t s_wave[SCAN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int first = 0; first < nblocks; first += SCAN_THREADS) {
    const int b = first + (int)threadIdx.x;
    const uint32_t v = b < nblocks ? counts[b] : 0u;
    uint32_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; ++w) {
      const uint32_t t = s_wave[w];
      if (w < wave) before += t;
      total += t;
    }
    if (b < nblocks) offsets[b] = carry + before + (incl - v);
    carry += total;
    __syncthreads();   // s_wave is rewritten by the next turn
  }
  if (threadIdx.x == 0) {
    *count_dev = (int32_t)carry;
    if (count_host) *count_host = (int32_t)carry;
  }
}

// save_points3D's colour: `col * 255.` in float32, then the truncating cast of storePly's uint8 field; the input is clamped to
// [0,1] first (a NaN gives 0)
__device__ __forceinline__ uint8_t compact_rgb8(float x) {
  const float c = fminf(fmaxf(x, 0.0f), 1.0f);
  return (uint8_t)(c * 255.0f);
}

// grid ceil(n / COMPACT_BLOCK): the kept elements of block b go to rows offsets[b] .. in element order
__global__ __launch_bounds__(256) void k_compact_scatter(int64_t n, const uint8_t* __restrict__ overlap, const uint32_t* __restrict__ offsets,
                                                         const float* __restrict__ points, const float* __restrict__ images,
                                                         const float* __restrict__ conf, float* __restrict__ out_points,
                                                         uint8_t* __restrict__ out_rgb8, float* __restrict__ out_conf) {
  __shared__ uint32_t s_seg[COMPACT_ROUNDS * 4];   // kept elements of (round, wave), then their exclusive prefix
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t base = (int64_t)blockIdx.x * COMPACT_BLOCK + threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  bool keep[COMPACT_ROUNDS];
  uint32_t rank[COMPACT_ROUNDS];
#pragma unroll
  for (int r = 0; r < COMPACT_ROUNDS; ++r) {
    keep[r] = compact_keep(base + r * 256, n, overlap);
    const unsigned long long m = __ballot(keep[r]);
    rank[r] = (uint32_t)__popcll(m & below);
    if (lane == 0) s_seg[r * 4 + wave] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = offsets[blockIdx.x];
    for (int k = 0; k < COMPACT_ROUNDS * 4; ++k) { const uint32_t c = s_seg[k]; s_seg[k] = run; run += c; }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < COMPACT_ROUNDS; ++r) {
    if (!keep[r]) continue;
    const size_t e = (size_t)(base + r * 256), o = (size_t)s_seg[r * 4 + wave] + rank[r];
    out_points[3 * o] = points[3 * e];
    out_points[3 * o + 1] = points[3 * e + 1];
    out_points[3 * o + 2] = points[3 * e + 2];
    out_rgb8[3 * o] = compact_rgb8(images[3 * e]);
    out_rgb8[3 * o + 1] = compact_rgb8(images[3 * e + 1]);
    out_rgb8[3 * o + 2] = compact_rgb8(images[3 * e + 2]);
    out_conf[o] = conf[e];
  }
}

// V <= 256 (the ranking travels in the kernel arguments, the pairs in grid.y), V H W <= 2^31 - 1 (an element's index is an
// int), H W small enough that the statistics pass' last workgroup stays inside an int
bool init_size_ok(int V, int H, int W) {
  if (V <= 0 || H <= 0 || W <= 0 || V > MAX_VIEWS) return false;
  if ((long long)H * W > 0x7fffffffLL - STATS_CHUNK) return false;
  return (long long)V * H * W <= 0x7fffffffLL;
}
int stats_chunks(int H, int W) { return (int)(((long long)H * W + STATS_CHUNK - 1) / STATS_CHUNK); }
bool compact_size_ok(int64_t n) { return n > 0 && n <= 0x7fffffffLL; }
int compact_blocks(int64_t n) { return (int)((n + COMPACT_BLOCK - 1) / COMPACT_BLOCK); }

}  // namespace

extern "C" {

size_t mi355gs_pointmap_stats_scratch_bytes(int V, int H, int W) {
  if (!init_size_ok(V, H, W)) return 0;
  return gs_align((size_t)V * stats_chunks(H, W) * sizeof(StatsPartial));
}

int mi355gs_pointmap_stats(void* stream_, int V, int H, int W, const float* depthmaps, const float* confidences, uint8_t* overlap,
                           void* scratch, double* stats) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!init_size_ok(V, H, W) || !depthmaps || !confidences || !overlap || !scratch || !stats) return MI355GS_EINVAL;
  const int chunks = stats_chunks(H, W);
  GS_KRANGE("pointmap_stats");
  hipLaunchKernelGGL(k_pointmap_stats, dim3(chunks, V), dim3(256), 0, stream, H * W, depthmaps, confidences, overlap,
                     (StatsPartial*)scratch);
  GS_CHECK_LAUNCH("pointmap_stats");
  GS_KRANGE("pointmap_stats_finish");
  hipLaunchKernelGGL(k_pointmap_stats_finish, dim3(V), dim3(256), 0, stream, chunks, (const StatsPartial*)scratch, stats);
  GS_CHECK_LAUNCH("pointmap_stats_finish");
  return MI355GS_OK;
}

int mi355gs_covis_masks(void* stream_, int V, int H, int W, const int32_t* order, const float* pointmaps, const float* depthmaps,
                        const float* intrinsics, const float* w2c, const double* stats, float depth_threshold, uint8_t* overlap) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!init_size_ok(V, H, W) || !order || !pointmaps || !depthmaps || !intrinsics || !w2c || !stats || !overlap) return MI355GS_EINVAL;
  ViewOrder vo;
  bool seen[MAX_VIEWS] = {false};
  for (int i = 0; i < V; ++i) {   // a permutation of 0 .. V-1
    if (order[i] < 0 || order[i] >= V || seen[order[i]]) return MI355GS_EINVAL;
    seen[order[i]] = true;
    vo.v[i] = (uint8_t)order[i];
  }
  for (int i = V; i < MAX_VIEWS; ++i) vo.v[i] = 0;
  if (V == 1) return MI355GS_OK;   // no pair: the first-ranked view is never marked
  const long long hw = (long long)H * W;
  GS_KRANGE("covis_masks");
  hipLaunchKernelGGL(k_covis_masks, dim3((unsigned)((hw + 255) / 256), (unsigned)(V * (V - 1) / 2)), dim3(256), 0, stream, W, H, vo,
                     pointmaps, depthmaps, intrinsics, w2c, stats, depth_threshold, overlap);
  GS_CHECK_LAUNCH("covis_masks");
  return MI355GS_OK;
}

size_t mi355gs_compact_scratch_bytes(int64_t n) {
  if (!compact_size_ok(n)) return 0;
  return gs_align((size_t)compact_blocks(n) * sizeof(uint32_t));
}

int mi355gs_compact_pointmaps(void* stream_, int64_t n, const uint8_t* overlap, const float* pointmaps, const float* images,
                              const float* confidences, void* scratch, float* out_points, uint8_t* out_rgb8, float* out_confidence,
                              int32_t* count_dev, int32_t* count_host) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!compact_size_ok(n) || !pointmaps || !images || !confidences || !scratch || !out_points || !out_rgb8 || !out_confidence || !count_dev)
    return MI355GS_EINVAL;
  const int nblocks = compact_blocks(n);
  uint32_t* counts = (uint32_t*)scratch;
  GS_KRANGE("compact_count");
  hipLaunchKernelGGL(k_compact_count, dim3(nblocks), dim3(256), 0, stream, n, overlap, counts);
  GS_CHECK_LAUNCH("compact_count");
  GS_KRANGE("compact_scan");
  hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(SCAN_THREADS), 0, stream, nblocks, (const uint32_t*)counts, counts, count_dev, count_host);
  GS_CHECK_LAUNCH("compact_scan");
  GS_KRANGE("compact_scatter");
  hipLaunchKernelGGL(k_compact_scatter, dim3(nblocks), dim3(256), 0, stream, n, overlap, (const uint32_t*)counts, pointmaps, images,
                     confidences, out_points, out_rgb8, out_confidence);
  GS_CHECK_LAUNCH("compact_scatter");
  return MI355GS_OK;
}

}  // extern "C"
