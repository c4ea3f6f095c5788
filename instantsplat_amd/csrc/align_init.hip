// The aligner's initialisation behind library calls (include/mi355gs.h, mi355gs_align_init_* and friends): the arithmetic of
// reference dust3r/cloud_opt/init_im_poses.py:66-221 (`init_minimum_spanning_tree`, `init_from_pts3d`) and
// dust3r/post_process.py:36-53 (the Weiszfeld focal).  Which record feeds which image — the tree and the walk over it — is decided
// on the host (instantsplat_amd/global_align.py); every sum over the H W points of a pointmap runs here.
//
//   row means      the 2 E confidence means behind the edge scores
//   registration   y ~ s R x + T for a batch of jobs (source pointmap, target pointmap, weights): two passes over the points —
//                  weighted centroids, then second moments of the CENTRED points (raw float32 moments cancel at depths of 2-5 with
//                  spreads under 1) — each leaving one partial row per workgroup, and per job one workgroup that adds the rows in
//                  a fixed order in double and, behind the second pass, solves the 3 x 3 Procrustes problem (one-sided Jacobi
//                  SVD, reflection fix) in double
//   apply          dst = s R src + T
//   focals         the closed-form start and the 10 re-weightings, one (sums, finish) pair of launches each, batched over images
//   state          scale normalisation, depth_log, im_pose, focal_log
//
// Stateless: the caller hands in the workspace (mi355gs_align_init_workspace_bytes).  No float atomics, no memset, no allocation,
// no host synchronisation: two calls give the same bits.  Contraction as for align.hip (Makefile): results are held to measured
// tolerances against float64, not to the reference's bits.
#include <math.h>
#include <float.h>
#include "common.h"

namespace {

constexpr int INIT_PPT = 4;                     // points per thread
constexpr int INIT_BLOCK = 256 * INIT_PPT;      // points of one job per workgroup of a sums kernel
constexpr int ROW = 12;                         // floats of one partial row (7, 10 or 2 of them used)
constexpr int MAX_JOBS = 65535;                 // grid.y
constexpr int MAX_VIEWS = 256;
constexpr int WEISZFELD_ITERS = 10;             // post_process.py:47
constexpr double FOCAL_BREAK = 20.0;            // optimizer.py:22

struct InitWs {
  float* part;       // [B][nchunk][ROW]
  double* centroid;  // [B][8]: sum w, centroid of the source [3], of the target [3]
  double* factor;    // [2]: the scale normalisation factor (state)
  float* cam;        // [MAX_VIEWS][16]: R [9], T [3] of every image (state)
};

int chunks_of(int n) { return (int)(((long long)n + INIT_BLOCK - 1) / INIT_BLOCK); }

size_t carve(InitWs& w, void* workspace, int B, int n) {
  GsCarver c{(char*)workspace};
  w.part = c.take<float>((size_t)B * (size_t)chunks_of(n) * ROW);
  w.centroid = c.take<double>((size_t)B * 8);
  w.factor = c.take<double>(2);
  w.cam = c.take<float>((size_t)MAX_VIEWS * 16);
  return c.off;
}

bool init_size_ok(int B, int n) {
  if (B <= 0 || n <= 0 || B > MAX_JOBS) return false;
  if ((long long)n > 0x7fffffffLL - INIT_BLOCK) return false;   // a sums kernel's last workgroup stays inside an int
  return (long long)B * n <= 0x7fffffffLL;
}

struct Job {   // one side of a batch: job b reads base + (idx ? idx[b] : b) * job_stride, a point every pt_stride floats
  const float* base;
  const int32_t* idx;
  long long job_stride;
  int pt_stride;
};
__device__ __forceinline__ const float* job_ptr(const Job& j, unsigned b) {
  return j.base + (size_t)(j.idx ? j.idx[b] : (int32_t)b) * (size_t)j.job_stride;
}

// The sum over the workgroup's four waves of COUNT values per thread -> row[0 .. COUNT) of this workgroup's partial row.
// Every thread of the workgroup must call it (DPP wave sums need all lanes).
template <int COUNT>
__device__ __forceinline__ void block_row(const float* vals, float* __restrict__ row) {
  __shared__ float s_red[4][ROW];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < COUNT; ++c) {
    const float t = gs_wave_sum_row3(vals[c]);
    if ((threadIdx.x & 63) == 63) s_red[wave][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < ROW)
    row[threadIdx.x] = threadIdx.x < COUNT ? (s_red[0][threadIdx.x] + s_red[1][threadIdx.x]) + (s_red[2][threadIdx.x] + s_red[3][threadIdx.x]) : 0.f;
}

// The rows of job `b` added in a fixed order, in double (k_align_reduce's scheme: thread (group g = t / 16, column c = t % 16)
// takes the rows g, g + 16, ..., then the 16 groups are added in sequence).  256 threads; the totals are valid in EVERY thread.
__device__ __forceinline__ void reduce_rows(const float* __restrict__ rows, int nchunk, int width, double* tot /* [ROW] */) {
  __shared__ double s_g[16][17];
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  double t = 0.0;
  if (c < width)
    for (int r = g; r < nchunk; r += 16) t += (double)rows[(size_t)r * ROW + c];
  s_g[g][c] = t;
  __syncthreads();
  for (int k = 0; k < width; ++k) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += s_g[q][k];
    tot[k] = s;
  }
  __syncthreads();   // s_g may be rewritten by the next call
}

// ---------------------------------------------------------------------------------------------------------------- row means
// grid (nchunk, rows)
__global__ __launch_bounds__(256) void k_init_mean_sums(int n, const float* __restrict__ x, float* __restrict__ part) {
  const float* __restrict__ row = x + (size_t)blockIdx.y * (size_t)n;
  const int first = (int)blockIdx.x * INIT_BLOCK + (int)threadIdx.x;
  float v[1] = {0.f};
#pragma unroll
  for (int j = 0; j < INIT_PPT; ++j) {
    const int p = first + j * 256;
    if (p < n) v[0] += row[p];
  }
  block_row<1>(v, part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ROW);
}
// grid rows
__global__ __launch_bounds__(256) void k_init_mean_finish(int n, int nchunk, const float* __restrict__ part, float* __restrict__ means) {
  double tot[ROW];
  reduce_rows(part + (size_t)blockIdx.x * nchunk * ROW, nchunk, 1, tot);
  if (threadIdx.x == 0) means[blockIdx.x] = (float)(tot[0] / (double)n);
}

// ---------------------------------------------------------------------------------------------------------------- registration
struct RegArgs {
  int n, nchunk;
  Job src, tgt, w;     // w.base null: unit weights
  float* part;
  double* centroid;
  float* srt;          // [B][16]: s, R row-major [9], T [3], 0 x 3
  float* pw_pose;      // [B][8] or null: quaternion (x y z w) of R, signed_log1p(T / s), log s
};

// grid (nchunk, B).  Pass 1: sum w, sum w (x - x0), sum w (y - y0) with (x0, y0) the job's first points as the pivot.
// Pass 2: sum w yh (x) xh [9] and sum w |xh|^2 with xh = x - centroid, yh = y - centroid.
template <int PASS>
__global__ __launch_bounds__(256) void k_init_reg_sums(RegArgs a) {
  const unsigned b = blockIdx.y;
  const float* __restrict__ xs = job_ptr(a.src, b);
  const float* __restrict__ ys = job_ptr(a.tgt, b);
  const float* __restrict__ ws = a.w.base ? job_ptr(a.w, b) : nullptr;
  const int sx = a.src.pt_stride, sy = a.tgt.pt_stride;
  float ox[3], oy[3];
  if (PASS == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { ox[c] = xs[c]; oy[c] = ys[c]; }
  } else {
    const double* __restrict__ cen = a.centroid + 8 * (size_t)b;
#pragma unroll
    for (int c = 0; c < 3; ++c) { ox[c] = (float)cen[1 + c]; oy[c] = (float)cen[4 + c]; }
  }
  constexpr int COUNT = PASS == 1 ? 7 : 10;
  float acc[COUNT];
#pragma unroll
  for (int c = 0; c < COUNT; ++c) acc[c] = 0.f;
  const int first = (int)blockIdx.x * INIT_BLOCK + (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < INIT_PPT; ++j) {
    const int p = first + j * 256;
    if (p >= a.n) continue;
    const float wt = ws ? ws[p] : 1.f;
    const float* __restrict__ xp = xs + (size_t)p * sx;
    const float* __restrict__ yp = ys + (size_t)p * sy;
    const float x0 = xp[0] - ox[0], x1 = xp[1] - ox[1], x2 = xp[2] - ox[2];
    const float y0 = yp[0] - oy[0], y1 = yp[1] - oy[1], y2 = yp[2] - oy[2];
    if (PASS == 1) {
      acc[0] += wt;
      acc[1] += wt * x0; acc[2] += wt * x1; acc[3] += wt * x2;
      acc[4] += wt * y0; acc[5] += wt * y1; acc[6] += wt * y2;
    } else {
      const float wy0 = wt * y0, wy1 = wt * y1, wy2 = wt * y2;
      acc[0] += wy0 * x0; acc[1] += wy0 * x1; acc[2] += wy0 * x2;
      acc[3] += wy1 * x0; acc[4] += wy1 * x1; acc[5] += wy1 * x2;
      acc[6] += wy2 * x0; acc[7] += wy2 * x1; acc[8] += wy2 * x2;
      acc[9] += wt * (x0 * x0 + x1 * x1 + x2 * x2);
    }
  }
  block_row<COUNT>(acc, a.part + ((size_t)b * a.nchunk + blockIdx.x) * ROW);
}

// A = U diag(sig) V^T by one-sided Jacobi: the columns of A are rotated until they are orthogonal (they become U diag(sig)),
// V collects the rotations.
__device__ void jacobi_svd3(double A[3][3], double V[3][3]) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int r = 0; r < 3; ++r) { alpha += A[r][p] * A[r][p]; beta += A[r][q] * A[r][q]; gamma += A[r][p] * A[r][q]; }
        if (gamma == 0.0 || fabs(gamma) <= 1e-17 * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int r = 0; r < 3; ++r) {
          const double ap = A[r][p], aq = A[r][q];
          A[r][p] = c * ap - s * aq; A[r][q] = s * ap + c * aq;
          const double vp = V[r][p], vq = V[r][q];
          V[r][p] = c * vp - s * vq; V[r][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
}

__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// scalar-last unit quaternion of a rotation matrix (row-major): the branch of the largest of R00, R11, R22 and the trace, the
// first of equals (tests/golden/roma_standin.py documents the rule)
__device__ void rotmat_to_quat(const double* R, double* q) {
  const double d[3] = {R[0], R[4], R[8]}, trace = R[0] + R[4] + R[8];
  int choice = 0;
  double best = d[0];
  if (d[1] > best) { best = d[1]; choice = 1; }
  if (d[2] > best) { best = d[2]; choice = 2; }
  if (trace > best) choice = 3;
  if (choice == 3) {
    q[0] = R[7] - R[5]; q[1] = R[2] - R[6]; q[2] = R[3] - R[1]; q[3] = 1.0 + trace;
  } else {
    const int i = choice, j = (choice + 1) % 3, k = (choice + 2) % 3;
    q[i] = 1.0 - trace + 2.0 * R[4 * i];
    q[j] = R[3 * j + i] + R[3 * i + j];
    q[k] = R[3 * k + i] + R[3 * i + k];
    q[3] = R[3 * k + j] - R[3 * j + k];
  }
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int c = 0; c < 4; ++c) q[c] /= nrm;
}
__device__ __forceinline__ double signed_log1p(double x) {
  const double l = log1p(fabs(x));
  return x > 0.0 ? l : (x < 0.0 ? -l : x);
}

// The special-orthogonal Procrustes solution of M = sum w yh xh^T (roma's conventions): R = U diag(1, 1, det(U) det(V)) V^T and
// the sum of the signed singular values.  The third singular direction is never divided by its (possibly zero: coplanar points)
// singular value: with u3 = u1 x u2 and v3 = v1 x v2 both factors are rotations, R = U V^T, and the third signed singular value
// is u3^T M v3 — negative exactly where the reflection fix fires.
__device__ void procrustes3(const double* M, double* R, double& trace_signed) {
  double A[3][3], V[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) A[r][c] = M[3 * r + c];
  jacobi_svd3(A, V);
  double sig[3];
  for (int c = 0; c < 3; ++c) sig[c] = sqrt(A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c]);
  int o0 = 0, o1 = 1, o2 = 2, t;   // descending
  if (sig[o0] < sig[o1]) { t = o0; o0 = o1; o1 = t; }
  if (sig[o1] < sig[o2]) { t = o1; o1 = o2; o2 = t; }
  if (sig[o0] < sig[o1]) { t = o0; o0 = o1; o1 = t; }
  double u[3][3], v[3][3];   // u[k], v[k]: the k-th left / right singular vector
  for (int r = 0; r < 3; ++r) {
    u[0][r] = A[r][o0] / sig[o0]; u[1][r] = A[r][o1] / sig[o1];
    v[0][r] = V[r][o0]; v[1][r] = V[r][o1];
  }
  cross3(u[0], u[1], u[2]);
  cross3(v[0], v[1], v[2]);
  double s3 = 0.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) s3 += u[2][r] * M[3 * r + c] * v[2][c];
  trace_signed = sig[o0] + sig[o1] + s3;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[3 * r + c] = u[0][r] * v[0][c] + u[1][r] * v[1][c] + u[2][r] * v[2][c];
}

// grid B.  Pass 1: the centroids.  Pass 2: s, R, T and the pw_pose row.
template <int PASS>
__global__ __launch_bounds__(256) void k_init_reg_finish(RegArgs a) {
  const unsigned b = blockIdx.x;
  double tot[ROW];
  reduce_rows(a.part + (size_t)b * a.nchunk * ROW, a.nchunk, PASS == 1 ? 7 : 10, tot);
  if (threadIdx.x != 0) return;
  double* cen = a.centroid + 8 * (size_t)b;
  if (PASS == 1) {
    const float* xs = job_ptr(a.src, b);
    const float* ys = job_ptr(a.tgt, b);
    cen[0] = tot[0];
    for (int c = 0; c < 3; ++c) {
      cen[1 + c] = (double)xs[c] + tot[1 + c] / tot[0];
      cen[4 + c] = (double)ys[c] + tot[4 + c] / tot[0];
    }
    cen[7] = 0.0;
    return;
  }
  // the second moments were formed around the centroids ROUNDED to float: use the same points here
  double cx[3], cy[3], R[9], trace_signed;
  for (int c = 0; c < 3; ++c) { cx[c] = (double)(float)cen[1 + c]; cy[c] = (double)(float)cen[4 + c]; }
  procrustes3(tot, R, trace_signed);
  const double s = trace_signed / tot[9];
  double T[3];
  for (int r = 0; r < 3; ++r) T[r] = cy[r] - s * (R[3 * r] * cx[0] + R[3 * r + 1] * cx[1] + R[3 * r + 2] * cx[2]);
  float* o = a.srt + 16 * (size_t)b;
  o[0] = (float)s;
  for (int k = 0; k < 9; ++k) o[1 + k] = (float)R[k];
  for (int k = 0; k < 3; ++k) o[10 + k] = (float)T[k];
  o[13] = o[14] = o[15] = 0.f;
  if (a.pw_pose) {
    double q[4];
    rotmat_to_quat(R, q);
    float* p = a.pw_pose + 8 * (size_t)b;
    for (int k = 0; k < 4; ++k) p[k] = (float)q[k];
    for (int k = 0; k < 3; ++k) p[4 + k] = (float)signed_log1p(T[k] / s);
    p[7] = (float)log(s);
  }
}

// ---------------------------------------------------------------------------------------------------------------- apply
// grid ceil(n / 256): dst[p] = s R src[p] + T (srt null: a copy)
__global__ __launch_bounds__(256) void k_init_apply(int n, const float* __restrict__ src, int pt_stride, const float* __restrict__ srt,
                                                    float* __restrict__ dst) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n) return;
  const float* __restrict__ x = src + (size_t)p * pt_stride;
  float* __restrict__ o = dst + 3 * (size_t)p;
  if (!srt) { o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; return; }
  const float s = srt[0];
  o[0] = s * (srt[1] * x[0] + srt[2] * x[1] + srt[3] * x[2]) + srt[10];
  o[1] = s * (srt[4] * x[0] + srt[5] * x[1] + srt[6] * x[2]) + srt[11];
  o[2] = s * (srt[7] * x[0] + srt[8] * x[1] + srt[9] * x[2]) + srt[12];
}

// ---------------------------------------------------------------------------------------------------------------- focals
// grid (nchunk, B).  iter 0: the closed form's sums (unit weights); later: weights 1 / max(|px - f xy|, 1e-8) with f = focals[b].
__global__ __launch_bounds__(256) void k_init_focal_sums(int n, int nchunk, int W, int H, int iter, Job src, const float* __restrict__ focals,
                                                         float* __restrict__ part) {
  const unsigned b = blockIdx.y;
  const float* __restrict__ xs = job_ptr(src, b);
  const float f = iter ? focals[b] : 0.f;
  const float ppx = 0.5f * (float)W, ppy = 0.5f * (float)H;
  float acc[2] = {0.f, 0.f};
  const int first = (int)blockIdx.x * INIT_BLOCK + (int)threadIdx.x;
#pragma unroll
  for (int j = 0; j < INIT_PPT; ++j) {
    const int p = first + j * 256;
    if (p >= n) continue;
    const float* __restrict__ x = xs + (size_t)p * src.pt_stride;
    const int row = p / W, col = p - row * W;
    const float u = (float)col - ppx, v = (float)row - ppy;
    float a0 = x[0] / x[2], a1 = x[1] / x[2];
    if (!(fabsf(a0) <= FLT_MAX)) a0 = 0.f;   // nan_to_num(posinf = 0, neginf = 0): every non-finite value becomes 0
    if (!(fabsf(a1) <= FLT_MAX)) a1 = 0.f;
    float wt = 1.f;
    if (iter) {
      const float d0 = u - f * a0, d1 = v - f * a1;
      wt = 1.f / fmaxf(sqrtf(d0 * d0 + d1 * d1), 1e-8f);
    }
    acc[0] += wt * (a0 * u + a1 * v);
    acc[1] += wt * (a0 * a0 + a1 * a1);
  }
  block_row<2>(acc, part + ((size_t)b * nchunk + blockIdx.x) * ROW);
}
// grid B (the means' 1 / n cancels in the quotient)
__global__ __launch_bounds__(256) void k_init_focal_finish(int nchunk, int last, const float* __restrict__ part, float* __restrict__ focals) {
  double tot[ROW];
  reduce_rows(part + (size_t)blockIdx.x * nchunk * ROW, nchunk, 2, tot);
  if (threadIdx.x != 0) return;
  float f = (float)(tot[0] / tot[1]);
  if (last && f < 0.f) f = 0.f;   // focal.clip(min = 0): a NaN stays
  focals[blockIdx.x] = f;
}

// ---------------------------------------------------------------------------------------------------------------- state
struct StateArgs {
  int V, E, n;
  uint32_t norm;
  float base_scale;
  int focal_mode;            // 0: per image, 1: the mean of the V estimates, 2: `known_focal`
  float known_focal;
  const float* srt;          // rows of 16
  const int32_t* pose_row;   // [V]: the row of `srt` whose [R | T] is image v's pose; < 0: identity
  const float* focals;       // [V]
  const int32_t* focal_row;  // [V]: the entry of `focals` that is image v's; < 0: focal_log keeps the constructor's value
  const float* pw_pose;      // [E][8]
  float *pts3d, *depth_log, *im_pose, *focal_log;
  float default_focal_log;
  double* factor;
  float* cam;
};

// one workgroup of 256: the factor exp(log(base_scale) - mean(log-scales)), the pose and focal rows, the per-image tables
__global__ __launch_bounds__(256) void k_init_state_small(StateArgs a) {
  __shared__ double s_lds[4];
  __shared__ double s_out[2];
  double part = 0.0, fpart = 0.0;
  for (int e = threadIdx.x; e < a.E; e += 256) part += (double)a.pw_pose[8 * (size_t)e + 7];
  for (int v = threadIdx.x; v < a.V; v += 256)
    if (a.focal_mode == 1 && a.focal_row[v] >= 0) fpart += (double)a.focals[a.focal_row[v]];   // (the caller refuses a missing one)
  part = gs_wave_sum_row3(part);
  fpart = gs_wave_sum_row3(fpart);
  if ((threadIdx.x & 63) == 63) s_lds[threadIdx.x >> 6] = part;
  __syncthreads();
  if (threadIdx.x == 0) s_out[0] = ((s_lds[0] + s_lds[1]) + (s_lds[2] + s_lds[3])) / (double)a.E;
  __syncthreads();
  if ((threadIdx.x & 63) == 63) s_lds[threadIdx.x >> 6] = fpart;
  __syncthreads();
  if (threadIdx.x == 0) s_out[1] = ((s_lds[0] + s_lds[1]) + (s_lds[2] + s_lds[3])) / (double)a.V;
  __syncthreads();
  // float32 as the reference forms it: (log(base_scale) - mean).exp() on a float32 tensor
  const double factor = a.norm ? (double)expf((float)(log((double)a.base_scale) - s_out[0])) : 1.0;
  if (threadIdx.x == 0) a.factor[0] = factor;
  for (int v = threadIdx.x; v < a.V; v += 256) {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, T[3] = {0, 0, 0};
    if (a.pose_row[v] >= 0) {
      const float* r = a.srt + 16 * (size_t)a.pose_row[v];
      for (int k = 0; k < 9; ++k) R[k] = (double)r[1 + k];
      for (int k = 0; k < 3; ++k) T[k] = (double)(float)((double)r[10 + k] * factor);
    }
    float* c = a.cam + 16 * (size_t)v;
    for (int k = 0; k < 9; ++k) c[k] = (float)R[k];
    for (int k = 0; k < 3; ++k) c[9 + k] = (float)T[k];
    c[12] = c[13] = c[14] = c[15] = 0.f;
    double q[4];
    rotmat_to_quat(R, q);
    float* p = a.im_pose + 7 * (size_t)v;
    for (int k = 0; k < 4; ++k) p[k] = (float)q[k];
    for (int k = 0; k < 3; ++k) p[4 + k] = (float)signed_log1p(T[k]);
    double focal = -1.0;
    if (a.focal_mode == 2) focal = (double)a.known_focal;
    else if (a.focal_mode == 1) focal = s_out[1];
    else if (a.focal_row[v] >= 0) focal = (double)a.focals[a.focal_row[v]];
    a.focal_log[v] = (a.focal_mode == 0 && a.focal_row[v] < 0) ? a.default_focal_log : (float)(FOCAL_BREAK * log(focal));
  }
}

// grid (ceil(n / 256), V): pts3d *= factor; depth_log = log(z of inv(pose) pts3d) with NaN and -inf -> 0, +inf -> FLT_MAX
__global__ __launch_bounds__(256) void k_init_state_depth(StateArgs a) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= a.n) return;
  const float* __restrict__ c = a.cam + 16 * blockIdx.y;
  const float factor = (float)a.factor[0];
  const size_t idx = (size_t)blockIdx.y * (size_t)a.n + (size_t)p;
  float* __restrict__ x = a.pts3d + 3 * idx;
  const float x0 = x[0] * factor, x1 = x[1] * factor, x2 = x[2] * factor;
  x[0] = x0; x[1] = x1; x[2] = x2;
  const float z = c[2] * (x0 - c[9]) + c[5] * (x1 - c[10]) + c[8] * (x2 - c[11]);   // the third row of R^T (X - T)
  float l = logf(z);
  if (!(l == l) || l == -INFINITY) l = 0.f;
  else if (l == INFINITY) l = FLT_MAX;
  a.depth_log[idx] = l;
}

Job make_job(const float* base, const int32_t* idx, long long job_stride, int pt_stride) {
  Job j;
  j.base = base; j.idx = idx; j.job_stride = job_stride; j.pt_stride = pt_stride;
  return j;
}

}  // namespace

extern "C" {

size_t mi355gs_align_init_workspace_bytes(int B, int n) {
  if (!init_size_ok(B, n)) return 0;
  InitWs w;
  return carve(w, nullptr, B, n);
}

int mi355gs_align_init_means(void* workspace, void* stream_, int rows, int n, const float* x, float* means) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!workspace || !x || !means || !init_size_ok(rows, n)) return MI355GS_EINVAL;
  InitWs w;
  carve(w, workspace, rows, n);
  const int nchunk = chunks_of(n);
  GS_KRANGE("align_init_mean_sums");
  hipLaunchKernelGGL(k_init_mean_sums, dim3(nchunk, rows), dim3(256), 0, stream, n, x, w.part);
  GS_CHECK_LAUNCH("align_init_mean_sums");
  GS_KRANGE("align_init_mean_finish");
  hipLaunchKernelGGL(k_init_mean_finish, dim3(rows), dim3(256), 0, stream, n, nchunk, (const float*)w.part, means);
  GS_CHECK_LAUNCH("align_init_mean_finish");
  return MI355GS_OK;
}

int mi355gs_align_init_register(void* workspace, void* stream_, int B, int n, const float* src, const int32_t* src_idx, long long src_job_stride,
                                int src_pt_stride, const float* tgt, const int32_t* tgt_idx, long long tgt_job_stride, const float* weights,
                                const int32_t* w_idx, long long w_job_stride, float* srt, float* pw_pose) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!workspace || !src || !tgt || !srt || !init_size_ok(B, n)) return MI355GS_EINVAL;
  if (src_pt_stride < 3 || src_pt_stride > 4 || src_job_stride < 0 || tgt_job_stride < 0 || w_job_stride < 0) return MI355GS_EINVAL;
  InitWs w;
  carve(w, workspace, B, n);
  RegArgs a;
  a.n = n; a.nchunk = chunks_of(n);
  a.src = make_job(src, src_idx, src_job_stride, src_pt_stride);
  a.tgt = make_job(tgt, tgt_idx, tgt_job_stride, 3);
  a.w = make_job(weights, w_idx, w_job_stride, 1);
  a.part = w.part; a.centroid = w.centroid; a.srt = srt; a.pw_pose = pw_pose;
  GS_KRANGE("align_init_reg_sums1");
  hipLaunchKernelGGL(k_init_reg_sums<1>, dim3(a.nchunk, B), dim3(256), 0, stream, a);
  GS_CHECK_LAUNCH("align_init_reg_sums1");
  GS_KRANGE("align_init_reg_finish1");
  hipLaunchKernelGGL(k_init_reg_finish<1>, dim3(B), dim3(256), 0, stream, a);
  GS_CHECK_LAUNCH("align_init_reg_finish1");
  GS_KRANGE("align_init_reg_sums2");
  hipLaunchKernelGGL(k_init_reg_sums<2>, dim3(a.nchunk, B), dim3(256), 0, stream, a);
  GS_CHECK_LAUNCH("align_init_reg_sums2");
  GS_KRANGE("align_init_reg_finish2");
  hipLaunchKernelGGL(k_init_reg_finish<2>, dim3(B), dim3(256), 0, stream, a);
  GS_CHECK_LAUNCH("align_init_reg_finish2");
  return MI355GS_OK;
}

int mi355gs_align_init_apply(void* stream_, int n, const float* src, int src_pt_stride, const float* srt, float* dst) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!src || !dst || !init_size_ok(1, n) || src_pt_stride < 3 || src_pt_stride > 4) return MI355GS_EINVAL;
  GS_KRANGE("align_init_apply");
  hipLaunchKernelGGL(k_init_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, src, src_pt_stride, srt, dst);
  GS_CHECK_LAUNCH("align_init_apply");
  return MI355GS_OK;
}

int mi355gs_align_init_focals(void* workspace, void* stream_, int B, int H, int W, const float* src, const int32_t* src_idx,
                              long long src_job_stride, int src_pt_stride, float* focals) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!workspace || !src || !focals || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || !init_size_ok(B, H * W)) return MI355GS_EINVAL;
  if (src_pt_stride < 3 || src_pt_stride > 4 || src_job_stride < 0) return MI355GS_EINVAL;
  const int n = H * W, nchunk = chunks_of(n);
  InitWs w;
  carve(w, workspace, B, n);
  const Job job = make_job(src, src_idx, src_job_stride, src_pt_stride);
  for (int iter = 0; iter <= WEISZFELD_ITERS; ++iter) {
    GS_KRANGE("align_init_focal_sums");
    hipLaunchKernelGGL(k_init_focal_sums, dim3(nchunk, B), dim3(256), 0, stream, n, nchunk, W, H, iter, job, (const float*)focals, w.part);
    GS_CHECK_LAUNCH("align_init_focal_sums");
    GS_KRANGE("align_init_focal_finish");
    hipLaunchKernelGGL(k_init_focal_finish, dim3(B), dim3(256), 0, stream, nchunk, iter == WEISZFELD_ITERS ? 1 : 0, (const float*)w.part, focals);
    GS_CHECK_LAUNCH("align_init_focal_finish");
  }
  return MI355GS_OK;
}

int mi355gs_align_init_state(void* workspace, void* stream_, int V, int E, int H, int W, int norm_pw_scale, float base_scale, int focal_mode,
                             float known_focal, const float* srt, const int32_t* pose_row, const float* focals, const int32_t* focal_row,
                             const float* pw_pose, float* pts3d, float* depth_log, float* im_pose, float* focal_log) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!workspace || !srt || !pose_row || !focals || !focal_row || !pw_pose || !pts3d || !depth_log || !im_pose || !focal_log) return MI355GS_EINVAL;
  if (V <= 0 || V > MAX_VIEWS || E <= 0 || E > MAX_JOBS || H <= 0 || W <= 0 || (long long)H * W > 0x7fffffffLL || !init_size_ok(V, H * W))
    return MI355GS_EINVAL;
  if (focal_mode < 0 || focal_mode > 2 || !(base_scale > 0.f) || (focal_mode == 2 && !(known_focal > 0.f))) return MI355GS_EINVAL;
  InitWs w;
  carve(w, workspace, V, H * W);
  StateArgs a;
  a.V = V; a.E = E; a.n = H * W;
  a.norm = norm_pw_scale ? 1u : 0u; a.base_scale = base_scale; a.focal_mode = focal_mode; a.known_focal = known_focal;
  a.srt = srt; a.pose_row = pose_row; a.focals = focals; a.focal_row = focal_row; a.pw_pose = pw_pose;
  a.pts3d = pts3d; a.depth_log = depth_log; a.im_pose = im_pose; a.focal_log = focal_log;
  a.default_focal_log = (float)(FOCAL_BREAK * log((double)(H > W ? H : W)));   // optimizer.py:38
  a.factor = w.factor; a.cam = w.cam;
  GS_KRANGE("align_init_state_small");
  hipLaunchKernelGGL(k_init_state_small, dim3(1), dim3(256), 0, stream, a);
  GS_CHECK_LAUNCH("align_init_state_small");
  GS_KRANGE("align_init_state_depth");
  hipLaunchKernelGGL(k_init_state_depth, dim3((unsigned)((a.n + 255) / 256), (unsigned)V), dim3(256), 0, stream, a);
  GS_CHECK_LAUNCH("align_init_state_depth");
  return MI355GS_OK;
}

}  // extern "C"
