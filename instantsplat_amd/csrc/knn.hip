// simple-knn: mean squared distance to the 3 nearest other points.
// replaces simple_knn._C.distCUDA2 at reference scene/gaussian_model.py:156 (one call per scene, at
// initialisation).  Exact 3-NN; neighbours are excluded by index, so duplicate points give 0
// (the caller clamps at 1e-7, same line of the reference).
//
// The reference operator sorts points along a Morton curve and prunes 1024-point boxes.  Here: a uniform grid
// over the bounding box (counting sort of the points by cell: count -> scan -> scatter, 3 launches), then one
// thread per point walks cubic shells of cells outwards from its own cell and stops as soon as its current
// third-best distance is no larger than the distance to the shell it has fully covered (less a margin for the rounding of
// the cell indices, see k_knn_query) — exact: the three smallest of the computed squared distances, O(N) memory,
// ~1 ms for 200k points instead of 25 ms for the exhaustive search (which is kept as the fallback for points
// whose search has not terminated after KNN_MAX_RING shells, e.g. far outliers, and for tiny clouds).
#include "common.h"

namespace {

constexpr int KNN_MAX_RING = 6;
constexpr float KNN_BIG = 3.402823466e38f;
constexpr float KNN_REACH = 1.0f - 1e-4f;

struct KnnGrid {
  float minx, miny, minz, inv_h, h;
  int gx, gy, gz;
};

__device__ __forceinline__ void knn_insert(float d, float& b0, float& b1, float& b2) {
  if (d < b2) {
    if (d < b1) {
      b2 = b1;
      if (d < b0) { b1 = b0; b0 = d; } else { b1 = d; }
    } else {
      b2 = d;
    }
  }
}

// Bounding box.  Workgroup b reduces the points b * 1024 + t, (b + gridDim.x) * 1024 + t, ... and writes (lo, hi) = two
// 3-float points at out + 6 b; a second launch with one workgroup over those 2 * gridDim.x points gives the box itself
// (one workgroup over all points was 103 us of a 280 us init at 196k points, 514 us at 1M).
__global__ __launch_bounds__(1024) void k_knn_bbox(int N, const float* __restrict__ pts, float* __restrict__ out /*[gridDim.x][6]*/) {
  __shared__ float s_red[16][6];
  float lo[3] = {KNN_BIG, KNN_BIG, KNN_BIG}, hi[3] = {-KNN_BIG, -KNN_BIG, -KNN_BIG};
  for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < (size_t)N; i += (size_t)gridDim.x * 1024)
#pragma unroll
    for (int k = 0; k < 3; ++k) { const float v = pts[3 * i + k]; lo[k] = fminf(lo[k], v); hi[k] = fmaxf(hi[k], v); }
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], m)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], m)); }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) { s_red[wave][k] = lo[k]; s_red[wave][3 + k] = hi[k]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    float v = s_red[0][k];
    for (int w = 1; w < 16; ++w) v = k < 3 ? fminf(v, s_red[w][k]) : fmaxf(v, s_red[w][k]);
    out[6 * (size_t)blockIdx.x + k] = v;
  }
}

__device__ __forceinline__ KnnGrid knn_grid(const float* __restrict__ bbox, int G) {
  KnnGrid g;
  g.minx = bbox[0]; g.miny = bbox[1]; g.minz = bbox[2];
  const float ex = bbox[3] - bbox[0], ey = bbox[4] - bbox[1], ez = bbox[5] - bbox[2];
  const float emax = fmaxf(fmaxf(ex, ey), fmaxf(ez, 1e-20f));
  g.h = emax / (float)G * 1.0001f;  // cubic cells; the longest axis gets G of them
  g.inv_h = 1.0f / g.h;
  g.gx = min(G, (int)(ex * g.inv_h) + 1); g.gy = min(G, (int)(ey * g.inv_h) + 1); g.gz = min(G, (int)(ez * g.inv_h) + 1);
  return g;
}

__device__ __forceinline__ void knn_cell_of(const KnnGrid& g, float x, float y, float z, int& cx, int& cy, int& cz) {
  cx = min(g.gx - 1, max(0, (int)((x - g.minx) * g.inv_h)));
  cy = min(g.gy - 1, max(0, (int)((y - g.miny) * g.inv_h)));
  cz = min(g.gz - 1, max(0, (int)((z - g.minz) * g.inv_h)));
}

__global__ __launch_bounds__(256) void k_knn_count(int N, int G, const float* __restrict__ pts, const float* __restrict__ bbox,
                                                    uint32_t* __restrict__ cell_count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const KnnGrid g = knn_grid(bbox, G);
  int cx, cy, cz;
  knn_cell_of(g, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], cx, cy, cz);
  atomicAdd(&cell_count[(cz * g.gy + cy) * g.gx + cx], 1u);
}

__global__ __launch_bounds__(256) void k_knn_scatter(int N, int G, const float* __restrict__ pts, const float* __restrict__ bbox,
                                                      const uint32_t* __restrict__ cell_start, uint32_t* __restrict__ cursor,
                                                      float4* __restrict__ sorted) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const KnnGrid g = knn_grid(bbox, G);
  const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
  int cx, cy, cz;
  knn_cell_of(g, x, y, z, cx, cy, cz);
  const int c = (cz * g.gy + cy) * g.gx + cx;
  const uint32_t pos = cell_start[c] + atomicAdd(&cursor[c], 1u);
  sorted[pos] = make_float4(x, y, z, __int_as_float(i));
}

__global__ __launch_bounds__(256) void k_knn_query(int N, int G, const float* __restrict__ bbox, const uint32_t* __restrict__ cell_start,
                                                    const float4* __restrict__ sorted, float* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;  // query = s-th point in cell order (neighbouring threads share cells)
  if (s >= N) return;
  const KnnGrid g = knn_grid(bbox, G);
  const float4 q = sorted[s];
  const int qi = __float_as_int(q.w);
  int cx, cy, cz;
  knn_cell_of(g, q.x, q.y, q.z, cx, cy, cz);
  float b0 = KNN_BIG, b1 = KNN_BIG, b2 = KNN_BIG;
  bool done = false;
  for (int r = 0; r <= KNN_MAX_RING && !done; ++r) {
    for (int dz = -r; dz <= r; ++dz) {
      const int z = cz + dz;
      if (z < 0 || z >= g.gz) continue;
      for (int dy = -r; dy <= r; ++dy) {
        const int y = cy + dy;
        if (y < 0 || y >= g.gy) continue;
        const bool face = (dz == -r || dz == r || dy == -r || dy == r);
        for (int dx = -r; dx <= r; dx += (face ? 1 : max(1, 2 * r))) {  // only the shell of the cube
          const int x = cx + dx;
          if (x < 0 || x >= g.gx) continue;
          const int c = (z * g.gy + y) * g.gx + x;
          const uint32_t lo = cell_start[c], hi = cell_start[c + 1];
          for (uint32_t j = lo; j < hi; ++j) {
            const float4 p = sorted[j];
            const float ex = p.x - q.x, ey = p.y - q.y, ez = p.z - q.z;
            if (__float_as_int(p.w) != qi) knn_insert(ex * ex + ey * ey + ez * ez, b0, b1, b2);
          }
        }
      }
    }
    // every point outside the (2r+1)^3 cube of cells is at least r*h away from q -- by the cells' real edges.  The indices
    // are the rounded (x - min) * inv_h, off by up to 3 * 2^-24 * G <= 4.6e-5 of a cell each, so two floats r + 1 cells apart
    // can be that much closer than r*h: the reach is shrunk by more than twice that (the mirror of the 1.0001 in h)
    const float reach = (float)r * g.h * KNN_REACH;
    done = b2 <= reach * reach;
  }
  if (!done) {  // far outlier or fewer than 4 points: exhaustive
    b0 = b1 = b2 = KNN_BIG;
    for (int j = 0; j < N; ++j) {
      const float4 p = sorted[j];
      const float ex = p.x - q.x, ey = p.y - q.y, ez = p.z - q.z;
      if (__float_as_int(p.w) != qi) knn_insert(ex * ex + ey * ey + ez * ez, b0, b1, b2);
    }
  }
  if (b0 == KNN_BIG) b0 = 0.f;  // fewer than 4 points: missing neighbours count as distance 0
  if (b1 == KNN_BIG) b1 = 0.f;
  if (b2 == KNN_BIG) b2 = 0.f;
  out[qi] = (b0 + b1 + b2) / 3.0f;
}

// grid resolution: points from pointmaps lie on surfaces, so ~sqrt(N/12) cells per axis gives a few points per
// occupied cell; capped so the cell table stays below 64 MiB
int knn_resolution(int N) {
  int G = 1;
  while ((long long)G * G * 12 < N && G < 256) ++G;
  return G < 4 ? 4 : G;
}

struct KnnLayout {
  size_t bbox, count, cursor, start, sorted, block_sums, total;
  int G;
  explicit KnnLayout(int N) {
    G = knn_resolution(N);
    const size_t cells = (size_t)G * G * G, n = N > 0 ? (size_t)N : 1;
    size_t o = 0;
    bbox = o; o += gs_align(6 * sizeof(float));
    count = o; o += gs_align(cells * 4);
    cursor = o; o += gs_align(cells * 4);
    start = o; o += gs_align((cells + 1) * 4);
    sorted = o; o += gs_align(n * sizeof(float4));
    block_sums = o; o += gs_align((cells / 4096 + 4) * 4);
    total = o;
  }
};

}  // namespace

extern "C" {

size_t mi355gs_knn_scratch_bytes(int N) { return KnnLayout(N).total + 256; }

int mi355gs_knn_dist2(void* stream_, int N, const float* points, float* mean_dist2, void* scratch) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (N < 0 || (N > 0 && (!points || !mean_dist2 || !scratch))) return MI355GS_EINVAL;
  if (N == 0) return MI355GS_OK;
  const KnnLayout L(N);
  char* w = (char*)scratch;
  float* bbox = (float*)(w + L.bbox);
  uint32_t* count = (uint32_t*)(w + L.count);
  uint32_t* cursor = (uint32_t*)(w + L.cursor);
  uint32_t* start = (uint32_t*)(w + L.start);
  float4* sorted = (float4*)(w + L.sorted);
  const int cells = L.G * L.G * L.G;
  if (hipMemsetAsync(count, 0, L.start - L.count, stream) != hipSuccess) return MI355GS_ELAUNCH;  // count + cursor
  const int bbox_blocks = min(1024, (N + 4095) / 4096);  // >= 4 points per thread
  if (bbox_blocks > 1) {  // partial boxes go to the (not yet used) sorted-points area: 24 B per workgroup <= 16 B per point
    hipLaunchKernelGGL(k_knn_bbox, dim3(bbox_blocks), dim3(1024), 0, stream, N, points, (float*)sorted);
    hipLaunchKernelGGL(k_knn_bbox, dim3(1), dim3(1024), 0, stream, 2 * bbox_blocks, (const float*)sorted, bbox);
  } else {
    GS_KRANGE("knn_bbox");
    hipLaunchKernelGGL(k_knn_bbox, dim3(1), dim3(1024), 0, stream, N, points, bbox);
  }
  GS_CHECK_LAUNCH("knn_bbox");
  const int blocks = (N + 255) / 256;
  GS_KRANGE("knn_count");
  hipLaunchKernelGGL(k_knn_count, dim3(blocks), dim3(256), 0, stream, N, L.G, points, (const float*)bbox, count);
  GS_CHECK_LAUNCH("knn_count");
  // exclusive scan over the cell table (cells that the tight per-axis grid does not use stay 0)
  GS_KRANGE("knn_scan");
  gs_launch_scan_large(stream, cells + 1, count, start, (uint32_t*)(w + L.block_sums), (int32_t*)(w + L.total));
  GS_CHECK_LAUNCH("knn_scan");
  GS_KRANGE("knn_scatter");
  hipLaunchKernelGGL(k_knn_scatter, dim3(blocks), dim3(256), 0, stream, N, L.G, points, (const float*)bbox, (const uint32_t*)start,
                     cursor, sorted);
  GS_CHECK_LAUNCH("knn_scatter");
  GS_KRANGE("knn_query");
  hipLaunchKernelGGL(k_knn_query, dim3(blocks), dim3(256), 0, stream, N, L.G, (const float*)bbox, (const uint32_t*)start,
                     (const float4*)sorted, mean_dist2);
  GS_CHECK_LAUNCH("knn_query");
  return MI355GS_OK;
}

}  // extern "C"
