// The global alignment loop behind library calls (include/mi355gs.h, mi355gs_align_*): reference
// dust3r/cloud_opt/base_opt.py:326-366 (`global_alignment_loop`) over dust3r/cloud_opt/optimizer.py:188-201
// (`PointCloudOptimizer.forward`) — per image a log-depth map, a camera pose and a focal, per directed edge a similarity
// transform, fitted with Adam to the network's pairwise pointmaps.
//
//   pack     once per problem: (x, y, z, log conf) of every edge side as one 16-byte record
//   prepare  once per call: the derived tables (per image R, T, focal, principal point; per edge sigma [R | T])
//   per iteration, 3 dispatches:
//     step    grid (workgroups of an image, V): one thread owns ALIGN_PPT pixels of one image.  Its world points are formed once
//             from one 4-byte log-depth each; it then walks every edge side at which the image occurs, one 16-byte load per
//             residual.  The depth gradient is complete in registers after the walk, so Adam is applied to the log-depth in
//             place (nobody else reads it; every shared parameter is only read in this launch).  Everything that feeds a small
//             parameter leaves as per-workgroup partial sums: 16 floats per image (13 pose / focal sums, the loss) and 12 per
//             edge side (dL/d(sigma [R | T])).
//     reduce  one workgroup per edge side and per image: its partial rows added in a fixed order, in double
//     finish  one workgroup: the chain through sigma, the mean coupling of norm_pw_scale, the quaternion normalisation and
//             signed_expm1; Adam on im_pose, focal_log and pw_pose; losses[k]; the derived tables of the next iteration
//
// No float atomics, no memset, no allocation, no host synchronisation inside a run: two runs give the same bits.
// Contraction (-ffp-contract) stays at hipcc's default: the trajectory is compared with a measured tolerance against a float64
// restatement, not bit for bit (Makefile).
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int ALIGN_PPT = 4;                      // pixels per thread
constexpr int ALIGN_BLOCK = 256 * ALIGN_PPT;      // pixels of one image per workgroup of the step kernel
constexpr int IMG_SUMS = 16;                      // G (x) c [9], G [3], focal sum, loss, 2 unused
constexpr int SIDE_SUMS = 12;                     // g (x) [a, 1], row-major 3x4
constexpr int FINISH_THREADS = 256;              // one workgroup; it loops over the edges and images
constexpr int MAX_VIEWS = 256;
constexpr int MAX_EDGES = 65535;
constexpr double FOCAL_BREAK = 20.0;              // reference optimizer.py:22
constexpr double PP_BREAK = 10.0;                 // reference optimizer.py:141-142

struct Align {
  int V, H, W, E, flags, nwg;
  float base_scale;
  bool tables_ready;
  // host copies of the tables, uploaded by the handle's first call
  uint32_t *h_side_tab, *h_side_first, *h_edge_sides;
  // device
  float4* recs;            // [2 E][n]: record of (edge, side) at index 2 e + side, side 0 = i
  uint32_t* side_tab;      // [2 E]: the record index 2 e + side of every edge side, grouped by the image it belongs to
  uint32_t* side_first;    // [V + 1]: image v owns side_tab[side_first[v] .. side_first[v + 1])
  uint32_t* edge_sides;    // [E][2]: where edge e's i and j side sit in side_tab
  float* Mt;               // [E][12]: sigma [R | T], row-major 3x4
  float* cam;              // [V][16]: R [9], T [3], focal, ppx, ppy
  float* img_part;         // [V][nwg][IMG_SUMS]
  float* side_part;        // [2 E][nwg][SIDE_SUMS]
  double* img_sums;        // [V][IMG_SUMS]
  double* side_sums;       // [2 E][SIDE_SUMS]
  double* dsig;            // [E]: dL/dsigma_e * sigma_e
};

size_t carve(Align& a, void* workspace) {
  GsCarver c{(char*)workspace};
  const size_t n = (size_t)a.H * a.W, E = (size_t)a.E, V = (size_t)a.V, nwg = (size_t)a.nwg;
  a.recs = c.take<float4>(2 * E * n);
  a.side_tab = c.take<uint32_t>(2 * E);
  a.side_first = c.take<uint32_t>(V + 1);
  a.edge_sides = c.take<uint32_t>(2 * E);
  a.Mt = c.take<float>(12 * E);
  a.cam = c.take<float>(16 * V);
  a.img_part = c.take<float>(V * nwg * IMG_SUMS);
  a.side_part = c.take<float>(2 * E * nwg * SIDE_SUMS);
  a.img_sums = c.take<double>(V * IMG_SUMS);
  a.side_sums = c.take<double>(2 * E * SIDE_SUMS);
  a.dsig = c.take<double>(E);
  return c.off;
}

bool align_size_ok(int V, int H, int W, int E, int flags) {
  if (V <= 0 || H <= 0 || W <= 0 || E <= 0 || V > MAX_VIEWS || E > MAX_EDGES) return false;
  if (flags < 0 || flags > 31) return false;
  if ((long long)H * W > 0x7fffffffLL - ALIGN_BLOCK) return false;   // the step kernel's last workgroup stays inside an int
  return (long long)E * H * W <= 0x7fffffffLL;
}

// torch.optim.Adam(betas = (0.9, 0.9), eps 1e-8, no weight decay) as torch runs it on a device tensor: lerp for the first moment,
// mul + addcmul for the second, denom = sqrt(v) / bc2_sqrt + eps, p += step_size * (m / denom) with step_size = -lr / bc1.
constexpr float ADAM_LERP_W = (float)(1.0 - 0.9);
constexpr float ADAM_BETA2 = (float)0.9;
constexpr float ADAM_ONE_MINUS_BETA2 = (float)(1.0 - 0.9);
constexpr float ADAM_EPS = (float)1e-8;

__device__ __forceinline__ float align_adam(float p, float g, float& m, float& v, float step_size, float bc2_sqrt) {
  m = fmaf(ADAM_LERP_W, g - m, m);
  v = fmaf(ADAM_ONE_MINUS_BETA2, g * g, v * ADAM_BETA2);
  const float denom = sqrtf(v) / bc2_sqrt + ADAM_EPS;
  return fmaf(step_size, m / denom, p);
}

// grid (ceil(n / 256), 2 E): record (e, side)[p] = (pred[e][p][0..2], log(conf[e][p]))
__global__ __launch_bounds__(256) void k_align_pack(int n, const float* __restrict__ pred_i, const float* __restrict__ pred_j,
                                                    const float* __restrict__ conf_i, const float* __restrict__ conf_j,
                                                    float4* __restrict__ recs) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n) return;
  const unsigned rs = blockIdx.y;
  const size_t src = (size_t)(rs >> 1) * (size_t)n + (size_t)p;
  const float* __restrict__ pred = (rs & 1u) ? pred_j : pred_i;
  const float* __restrict__ conf = (rs & 1u) ? conf_j : conf_i;
  recs[(size_t)rs * (size_t)n + (size_t)p] = make_float4(pred[3 * src], pred[3 * src + 1], pred[3 * src + 2], logf(conf[src]));
}

struct StepArgs {
  int n, W, nwg;
  uint32_t opt_depth;          // apply Adam to the log-depths (else, with g_depth set, store their gradient)
  float inv_En;                // 1 / (E n): the loss' normalisation
  const float4* recs;
  const uint32_t *side_tab, *side_first;
  const float *Mt, *cam;
  float *depth_log, *m_depth, *v_depth, *g_depth;
  const float4* sched;         // (step_size, bc2_sqrt, -, -) of this iteration, or null: no update
  float *img_part, *side_part;
};

// The sum over the workgroup's four waves of up to 16 values per wave (every lane active; totals land in lane 63):
// `slot` is this launch-phase's own LDS block, so consecutive phases need one barrier each.
template <int COUNT>
__device__ __forceinline__ void wave_totals_to_lds(const float* vals, float (*slot)[16]) {
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < COUNT; ++c) {
    const float t = gs_wave_sum_row3(vals[c]);
    if ((threadIdx.x & 63) == 63) slot[wave][c] = t;
  }
}

__global__ __launch_bounds__(256) void k_align_step(StepArgs a) {
  __shared__ float s_red[2][4][16];
  const int v = (int)blockIdx.y, n = a.n;
  const float* __restrict__ cam = a.cam + 16 * v;
  const float R0 = cam[0], R1 = cam[1], R2 = cam[2], R3 = cam[3], R4 = cam[4], R5 = cam[5], R6 = cam[6], R7 = cam[7], R8 = cam[8];
  const float T0 = cam[9], T1 = cam[10], T2 = cam[11], focal = cam[12], ppx = cam[13], ppy = cam[14];
  const size_t img = (size_t)v * (size_t)n;
  const int first = (int)blockIdx.x * ALIGN_BLOCK + (int)threadIdx.x;   // < n + ALIGN_BLOCK <= 2^31 - 1 + 1024: E n <= 2^31 - 1 and the
                                                                        // grid stops at ceil(n / ALIGN_BLOCK), so `first` < n + 256
  bool valid[ALIGN_PPT];
  float dl[ALIGN_PPT], d[ALIGN_PPT], ux[ALIGN_PPT], uy[ALIGN_PPT], X0[ALIGN_PPT], X1[ALIGN_PPT], X2[ALIGN_PPT];
  float G0[ALIGN_PPT], G1[ALIGN_PPT], G2[ALIGN_PPT];
#pragma unroll
  for (int j = 0; j < ALIGN_PPT; ++j) {
    const int p = first + j * 256;
    valid[j] = p < n;
    const int pc = valid[j] ? p : 0;
    const int row = pc / a.W, col = pc - row * a.W;
    dl[j] = a.depth_log[img + pc];
    d[j] = expf(dl[j]);
    ux[j] = (float)col - ppx;
    uy[j] = (float)row - ppy;
    const float cx = d[j] * ux[j] / focal, cy = d[j] * uy[j] / focal, cz = d[j];   // reference: depth * (grid - pp) / focal
    X0[j] = R0 * cx + R1 * cy + R2 * cz + T0;
    X1[j] = R3 * cx + R4 * cy + R5 * cz + T1;
    X2[j] = R6 * cx + R7 * cy + R8 * cz + T2;
    G0[j] = G1[j] = G2[j] = 0.f;
  }
  float loss = 0.f;
  const uint32_t s_begin = a.side_first[v], s_end = a.side_first[v + 1];
  float4 cur[ALIGN_PPT], nxt[ALIGN_PPT];
  {
    const size_t base = (size_t)a.side_tab[s_begin] * (size_t)n;   // every image has at least one side (checked at create)
#pragma unroll
    for (int j = 0; j < ALIGN_PPT; ++j) cur[j] = valid[j] ? a.recs[base + (size_t)(first + j * 256)] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (uint32_t s = s_begin; s < s_end; ++s) {
    const uint32_t rs = a.side_tab[s];
    if (s + 1 < s_end) {   // the next side's records are on their way while this side's are used
      const size_t base = (size_t)a.side_tab[s + 1] * (size_t)n;
#pragma unroll
      for (int j = 0; j < ALIGN_PPT; ++j) nxt[j] = valid[j] ? a.recs[base + (size_t)(first + j * 256)] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const float* __restrict__ M = a.Mt + 12 * (size_t)(rs >> 1);
    const float M0 = M[0], M1 = M[1], M2 = M[2], M3 = M[3], M4 = M[4], M5 = M[5], M6 = M[6], M7 = M[7], M8 = M[8], M9 = M[9],
                M10 = M[10], M11 = M[11];
    float acc[SIDE_SUMS];
#pragma unroll
    for (int c = 0; c < SIDE_SUMS; ++c) acc[c] = 0.f;
#pragma unroll
    for (int j = 0; j < ALIGN_PPT; ++j) {
      const float4 r = cur[j];   // (a, w); an invalid pixel has w = 0 and contributes nothing
      const float r0 = X0[j] - (M0 * r.x + M1 * r.y + M2 * r.z + M3);
      const float r1 = X1[j] - (M4 * r.x + M5 * r.y + M6 * r.z + M7);
      const float r2 = X2[j] - (M8 * r.x + M9 * r.y + M10 * r.z + M11);
      const float nrm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
      const float k = nrm > 0.f ? r.w / nrm : 0.f;   // the gradient of the norm at a zero residual is 0 (torch's norm backward)
      const float g0 = k * r0, g1 = k * r1, g2 = k * r2;
      loss += r.w * nrm;
      G0[j] += g0; G1[j] += g1; G2[j] += g2;
      acc[0] += g0 * r.x; acc[1] += g0 * r.y; acc[2] += g0 * r.z; acc[3] += g0;
      acc[4] += g1 * r.x; acc[5] += g1 * r.y; acc[6] += g1 * r.z; acc[7] += g1;
      acc[8] += g2 * r.x; acc[9] += g2 * r.y; acc[10] += g2 * r.z; acc[11] += g2;
    }
    float (*slot)[16] = s_red[(s - s_begin) & 1u];
    wave_totals_to_lds<SIDE_SUMS>(acc, slot);
    __syncthreads();   // one barrier per side: the slot of side s is rewritten by side s + 2, behind the barrier of side s + 1
    if (threadIdx.x < SIDE_SUMS)
      a.side_part[((size_t)s * (size_t)a.nwg + blockIdx.x) * SIDE_SUMS + threadIdx.x] =
          (slot[0][threadIdx.x] + slot[1][threadIdx.x]) + (slot[2][threadIdx.x] + slot[3][threadIdx.x]);
#pragma unroll
    for (int j = 0; j < ALIGN_PPT; ++j) cur[j] = nxt[j];
  }
  // per pixel: the gradient of its log-depth; per image: the sums behind dL/dR, dL/dT and dL/dfocal
  float sums[IMG_SUMS];
#pragma unroll
  for (int c = 0; c < IMG_SUMS; ++c) sums[c] = 0.f;
  float4 sc = make_float4(0.f, 1.f, 0.f, 0.f);
  const bool update = a.opt_depth && a.sched;
  if (update) sc = *a.sched;
#pragma unroll
  for (int j = 0; j < ALIGN_PPT; ++j) {
    const float cx = d[j] * ux[j] / focal, cy = d[j] * uy[j] / focal, cz = d[j];
    const float c0 = R0 * G0[j] + R3 * G1[j] + R6 * G2[j];   // R^T G: the gradient of the camera-frame point
    const float c1 = R1 * G0[j] + R4 * G1[j] + R7 * G2[j];
    const float c2 = R2 * G0[j] + R5 * G1[j] + R8 * G2[j];
    sums[0] += G0[j] * cx; sums[1] += G0[j] * cy; sums[2] += G0[j] * cz;
    sums[3] += G1[j] * cx; sums[4] += G1[j] * cy; sums[5] += G1[j] * cz;
    sums[6] += G2[j] * cx; sums[7] += G2[j] * cy; sums[8] += G2[j] * cz;
    sums[9] += G0[j]; sums[10] += G1[j]; sums[11] += G2[j];
    sums[12] += c0 * cx + c1 * cy;
    if (!valid[j]) continue;   // (an invalid pixel's G is 0: it added nothing above)
    const float gd = (c0 * (ux[j] / focal) + c1 * (uy[j] / focal) + c2) * d[j] * a.inv_En;
    const size_t idx = img + (size_t)(first + j * 256);
    if (update) {
      float m = a.m_depth[idx], vv = a.v_depth[idx];
      a.depth_log[idx] = align_adam(dl[j], gd, m, vv, sc.x, sc.y);
      a.m_depth[idx] = m; a.v_depth[idx] = vv;
    } else if (a.g_depth) {
      a.g_depth[idx] = gd;
    }
  }
  sums[13] = loss;
  float (*slot)[16] = s_red[(s_end - s_begin) & 1u];
  wave_totals_to_lds<14>(sums, slot);
  __syncthreads();
  if (threadIdx.x < IMG_SUMS)
    a.img_part[((size_t)v * (size_t)a.nwg + blockIdx.x) * IMG_SUMS + threadIdx.x] =
        threadIdx.x < 14 ? (slot[0][threadIdx.x] + slot[1][threadIdx.x]) + (slot[2][threadIdx.x] + slot[3][threadIdx.x]) : 0.f;
}

// grid 2 E + V, 256 threads: job < 2 E adds the nwg rows of 12 of edge side `job`, the others the rows of 16 of an image —
// thread (group g = t / 16, column c = t % 16) takes the rows g, g + 16, ... in double, then the 16 groups are added in sequence.
__global__ __launch_bounds__(256) void k_align_reduce(int n_sides, int nwg, const float* __restrict__ side_part,
                                                      const float* __restrict__ img_part, double* __restrict__ side_sums,
                                                      double* __restrict__ img_sums) {
  __shared__ double s_g[16][17];
  const int job = (int)blockIdx.x, c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const bool side = job < n_sides;
  const int width = side ? SIDE_SUMS : IMG_SUMS;
  const float* __restrict__ rows = side ? side_part + (size_t)job * nwg * SIDE_SUMS : img_part + (size_t)(job - n_sides) * nwg * IMG_SUMS;
  double t = 0.0;
  if (c < width)
    for (int r = g; r < nwg; r += 16) t += (double)rows[(size_t)r * width + c];
  s_g[g][c] = t;
  __syncthreads();
  if (threadIdx.x < (unsigned)width) {
    double tot = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) tot += s_g[q][threadIdx.x];
    (side ? side_sums + (size_t)job * SIDE_SUMS : img_sums + (size_t)(job - n_sides) * IMG_SUMS)[threadIdx.x] = tot;
  }
}

// the sum of one double per thread over FINISH_THREADS threads, in every thread; fixed order (DPP wave sum, the 16 wave totals
// in sequence).  Every thread must call it.
__device__ __forceinline__ double finish_block_sum(double v, double* lds /* [FINISH_THREADS / 64] */) {
  v = gs_wave_sum_row3(v);
  __syncthreads();   // lds may still be read from an earlier call
  if ((threadIdx.x & 63) == 63) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < FINISH_THREADS / 64; ++w) t += lds[w];
  return t;
}

struct Pose {   // a raw 7-vector (quaternion x y z w, then t) and what the reference's _get_poses makes of it
  double q[4], qn[4], norm, R[9], t[3], T[3];
};
__device__ __forceinline__ Pose load_pose7(const float* p) {
  Pose o;
#pragma unroll
  for (int c = 0; c < 4; ++c) o.q[c] = (double)p[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) o.t[c] = (double)p[4 + c];
  o.norm = sqrt(o.q[0] * o.q[0] + o.q[1] * o.q[1] + o.q[2] * o.q[2] + o.q[3] * o.q[3]);
#pragma unroll
  for (int c = 0; c < 4; ++c) o.qn[c] = o.q[c] / o.norm;
  const double x = o.qn[0], y = o.qn[1], z = o.qn[2], w = o.qn[3];
  o.R[0] = 1.0 - 2.0 * (y * y + z * z); o.R[1] = 2.0 * (x * y - w * z); o.R[2] = 2.0 * (x * z + w * y);
  o.R[3] = 2.0 * (x * y + w * z); o.R[4] = 1.0 - 2.0 * (x * x + z * z); o.R[5] = 2.0 * (y * z - w * x);
  o.R[6] = 2.0 * (x * z - w * y); o.R[7] = 2.0 * (y * z + w * x); o.R[8] = 1.0 - 2.0 * (x * x + y * y);
#pragma unroll
  for (int c = 0; c < 3; ++c) {   // signed_expm1
    const double e = expm1(fabs(o.t[c]));
    o.T[c] = o.t[c] > 0.0 ? e : (o.t[c] < 0.0 ? -e : 0.0);
  }
  return o;
}
// dL/d(raw 7-vector) from dL/dR (row-major 3x3) and dL/dT
__device__ __forceinline__ void pose7_backward(const Pose& o, const double* GR, const double* GT, double* out) {
  const double x = o.qn[0], y = o.qn[1], z = o.qn[2], w = o.qn[3];
  double gq[4];
  gq[0] = 2.0 * (y * (GR[1] + GR[3]) + z * (GR[2] + GR[6]) - 2.0 * x * (GR[4] + GR[8]) + w * (GR[7] - GR[5]));
  gq[1] = 2.0 * (x * (GR[1] + GR[3]) + z * (GR[5] + GR[7]) - 2.0 * y * (GR[0] + GR[8]) + w * (GR[2] - GR[6]));
  gq[2] = 2.0 * (x * (GR[2] + GR[6]) + y * (GR[5] + GR[7]) - 2.0 * z * (GR[0] + GR[4]) + w * (GR[3] - GR[1]));
  gq[3] = 2.0 * (z * (GR[3] - GR[1]) + y * (GR[2] - GR[6]) + x * (GR[7] - GR[5]));
  const double radial = gq[0] * x + gq[1] * y + gq[2] * z + gq[3] * w;   // normalisation: (I - qn qn^T) / |q|
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = (gq[c] - radial * o.qn[c]) / o.norm;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[4 + c] = o.t[c] != 0.0 ? GT[c] * exp(fabs(o.t[c])) : 0.0;   // d(sign(t) expm1|t|) = sign^2 exp|t|
}

struct FinishArgs {
  int V, E, H, W;
  uint32_t flags;
  float base_scale;
  double inv_En;
  const uint32_t* edge_sides;
  const double *side_sums, *img_sums;
  double* dsig;
  float *im_pose, *focal_log, *pw_pose;
  const float* pp_raw;
  float *m_im_pose, *v_im_pose, *m_focal, *v_focal, *m_pw_pose, *v_pw_pose;   // run
  float *g_im_pose, *g_focal, *g_pw_pose;                                     // grad
  const float4* sched;    // this iteration's (step_size, bc2_sqrt, -, -); null: no update
  float* loss_out;        // null: the prepare launch (tables only)
  float *Mt, *cam;
};

// The derived tables from the state as it stands: per image R, T, focal, principal point; per edge sigma [R | T] with
// sigma_e = exp(s_e) * exp(log(base_scale) - mean(s)) under norm_pw_scale, else exp(s_e).
__device__ __forceinline__ void derive_tables(const FinishArgs& a, double* lds) {
  double part = 0.0;
  for (int e = threadIdx.x; e < a.E; e += FINISH_THREADS) part += (double)a.pw_pose[8 * (size_t)e + 7];
  const double mean_s = finish_block_sum(part, lds) / (double)a.E;
  const double factor = (a.flags & MI355GS_ALIGN_NORM_PW_SCALE) ? exp(log((double)a.base_scale) - mean_s) : 1.0;
  for (int e = threadIdx.x; e < a.E; e += FINISH_THREADS) {
    const Pose o = load_pose7(a.pw_pose + 8 * (size_t)e);
    const double sigma = exp((double)a.pw_pose[8 * (size_t)e + 7]) * factor;
    float* M = a.Mt + 12 * (size_t)e;
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) M[4 * r + c] = (float)(sigma * o.R[3 * r + c]);
      M[4 * r + 3] = (float)(sigma * o.T[r]);
    }
  }
  for (int v = threadIdx.x; v < a.V; v += FINISH_THREADS) {
    const Pose o = load_pose7(a.im_pose + 7 * (size_t)v);
    float* c = a.cam + 16 * (size_t)v;
    for (int k = 0; k < 9; ++k) c[k] = (float)o.R[k];
    for (int k = 0; k < 3; ++k) c[9 + k] = (float)o.T[k];
    c[12] = (float)exp((double)a.focal_log[v] / FOCAL_BREAK);
    c[13] = (float)((double)a.W / 2.0 + PP_BREAK * (double)a.pp_raw[2 * v]);
    c[14] = (float)((double)a.H / 2.0 + PP_BREAK * (double)a.pp_raw[2 * v + 1]);
    c[15] = 0.f;
  }
}

// one workgroup.  The state pointers are neither const nor restrict: this launch reads what it has just written.
__global__ __launch_bounds__(FINISH_THREADS) void k_align_finish(FinishArgs a) {
  __shared__ double s_lds[FINISH_THREADS / 64];
  if (a.loss_out) {
    const bool update = a.sched != nullptr;
    float4 sc = make_float4(0.f, 1.f, 0.f, 0.f);
    if (update) sc = *a.sched;
    // dL/dsigma_e = sum_ij dL/dM_ij [R | T]_ij with dL/dM = -(S_i + S_j): the residual is X - M [a, 1]
    for (int e = threadIdx.x; e < a.E; e += FINISH_THREADS) {
      const Pose o = load_pose7(a.pw_pose + 8 * (size_t)e);
      const double* Si = a.side_sums + SIDE_SUMS * (size_t)a.edge_sides[2 * e];
      const double* Sj = a.side_sums + SIDE_SUMS * (size_t)a.edge_sides[2 * e + 1];
      double dsg = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) dsg -= (Si[4 * r + c] + Sj[4 * r + c]) * o.R[3 * r + c];
        dsg -= (Si[4 * r + 3] + Sj[4 * r + 3]) * o.T[r];
      }
      a.dsig[e] = dsg;
    }
    // sigma_e = exp(s_e) * factor from the state (the tables hold it only multiplied into R and T)
    double spart = 0.0;
    for (int e = threadIdx.x; e < a.E; e += FINISH_THREADS) spart += (double)a.pw_pose[8 * (size_t)e + 7];
    const double mean_s = finish_block_sum(spart, s_lds) / (double)a.E;
    const bool norm = (a.flags & MI355GS_ALIGN_NORM_PW_SCALE) != 0;
    const double factor = norm ? exp(log((double)a.base_scale) - mean_s) : 1.0;
    // dL/ds_k = dL/dsigma_k sigma_k - (1 / E) sum_e dL/dsigma_e sigma_e: the mean coupling of norm_pw_scale ties every s to all
    // the others (each thread rereads only the dsig entries it wrote itself)
    double wpart = 0.0;
    for (int e = threadIdx.x; e < a.E; e += FINISH_THREADS) {
      const double sigma = exp((double)a.pw_pose[8 * (size_t)e + 7]) * factor;
      a.dsig[e] *= sigma;
      wpart += a.dsig[e];
    }
    const double coupled = norm ? finish_block_sum(wpart, s_lds) / (double)a.E : 0.0;
    if ((a.flags & MI355GS_ALIGN_OPT_PW_POSES) || a.g_pw_pose) {
      for (int e = threadIdx.x; e < a.E; e += FINISH_THREADS) {
        float* p = a.pw_pose + 8 * (size_t)e;
        const Pose o = load_pose7(p);
        const double sigma = exp((double)p[7]) * factor;
        const double* Si = a.side_sums + SIDE_SUMS * (size_t)a.edge_sides[2 * e];
        const double* Sj = a.side_sums + SIDE_SUMS * (size_t)a.edge_sides[2 * e + 1];
        double GR[9], GT[3], g[8];
        for (int r = 0; r < 3; ++r) {
          for (int c = 0; c < 3; ++c) GR[3 * r + c] = -sigma * (Si[4 * r + c] + Sj[4 * r + c]);
          GT[r] = -sigma * (Si[4 * r + 3] + Sj[4 * r + 3]);
        }
        pose7_backward(o, GR, GT, g);
        g[7] = a.dsig[e] - coupled;
        for (int c = 0; c < 8; ++c) {
          const float gc = (float)(g[c] * a.inv_En);
          if (update && (a.flags & MI355GS_ALIGN_OPT_PW_POSES)) {
            float m = a.m_pw_pose[8 * (size_t)e + c], vv = a.v_pw_pose[8 * (size_t)e + c];
            p[c] = align_adam(p[c], gc, m, vv, sc.x, sc.y);
            a.m_pw_pose[8 * (size_t)e + c] = m; a.v_pw_pose[8 * (size_t)e + c] = vv;
          } else if (a.g_pw_pose) {
            a.g_pw_pose[8 * (size_t)e + c] = gc;
          }
        }
      }
    }
    double lpart = 0.0;
    for (int v = threadIdx.x; v < a.V; v += FINISH_THREADS) {
      const double* S = a.img_sums + IMG_SUMS * (size_t)v;
      lpart += S[13];
      float* p = a.im_pose + 7 * (size_t)v;
      const Pose o = load_pose7(p);
      double g[7];
      pose7_backward(o, S, S + 9, g);
      for (int c = 0; c < 7; ++c) {
        const float gc = (float)(g[c] * a.inv_En);
        if (update && (a.flags & MI355GS_ALIGN_OPT_IM_POSES)) {
          float m = a.m_im_pose[7 * (size_t)v + c], vv = a.v_im_pose[7 * (size_t)v + c];
          p[c] = align_adam(p[c], gc, m, vv, sc.x, sc.y);
          a.m_im_pose[7 * (size_t)v + c] = m; a.v_im_pose[7 * (size_t)v + c] = vv;
        } else if (a.g_im_pose) {
          a.g_im_pose[7 * (size_t)v + c] = gc;
        }
      }
      // focal = exp(focal_log / 20): the camera-frame x and y are d u / focal, so dL/dfocal_log = -S_f / 20
      const float gf = (float)(-S[12] / FOCAL_BREAK * a.inv_En);
      if (update && (a.flags & MI355GS_ALIGN_OPT_FOCALS)) {
        float m = a.m_focal[v], vv = a.v_focal[v];
        a.focal_log[v] = align_adam(a.focal_log[v], gf, m, vv, sc.x, sc.y);
        a.m_focal[v] = m; a.v_focal[v] = vv;
      } else if (a.g_focal) {
        a.g_focal[v] = gf;
      }
    }
    const double loss = finish_block_sum(lpart, s_lds) * a.inv_En;
    if (threadIdx.x == 0) *a.loss_out = (float)loss;
    if (!update) return;   // the gradient call leaves the state, and with it the tables, as they are
    __syncthreads();       // the tables below are derived from the state this workgroup has just stepped
  }
  derive_tables(a, s_lds);
}

// grid (ceil(n / 256), V): get_pts3d and get_depthmaps from the state and the tables of the prepare launch
__global__ __launch_bounds__(256) void k_align_points(int n, int W, const float* __restrict__ cam_all, const float* __restrict__ depth_log,
                                                      float* __restrict__ pts3d, float* __restrict__ depth) {
  const int p = (int)(blockIdx.x * 256u + threadIdx.x);
  if (p >= n) return;
  const float* __restrict__ cam = cam_all + 16 * blockIdx.y;
  const size_t idx = (size_t)blockIdx.y * (size_t)n + (size_t)p;
  const int row = p / W, col = p - row * W;
  const float d = expf(depth_log[idx]);
  const float cx = d * ((float)col - cam[13]) / cam[12], cy = d * ((float)row - cam[14]) / cam[12];
  pts3d[3 * idx] = cam[0] * cx + cam[1] * cy + cam[2] * d + cam[9];
  pts3d[3 * idx + 1] = cam[3] * cx + cam[4] * cy + cam[5] * d + cam[10];
  pts3d[3 * idx + 2] = cam[6] * cx + cam[7] * cy + cam[8] * d + cam[11];
  depth[idx] = d;
}

int upload_tables(Align* a, hipStream_t stream) {   // once, on the stream of the handle's first call; the host copies stay alive
  if (a->tables_ready) return MI355GS_OK;
  const size_t E = (size_t)a->E, V = (size_t)a->V;
  if (hipMemcpyAsync(a->side_tab, a->h_side_tab, 2 * E * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(a->side_first, a->h_side_first, (V + 1) * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipMemcpyAsync(a->edge_sides, a->h_edge_sides, 2 * E * 4, hipMemcpyHostToDevice, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess) {
    gs_log_error("align_tables", "copy of the edge-side tables failed");
    return MI355GS_ELAUNCH;
  }
  a->tables_ready = true;
  return MI355GS_OK;
}

FinishArgs finish_args(const Align* a, float* im_pose, float* focal_log, const float* pp_raw, float* pw_pose) {
  FinishArgs f;
  memset(&f, 0, sizeof(f));
  f.V = a->V; f.E = a->E; f.H = a->H; f.W = a->W;
  f.flags = (uint32_t)a->flags; f.base_scale = a->base_scale;
  f.inv_En = 1.0 / ((double)a->E * (double)a->H * (double)a->W);
  f.edge_sides = a->edge_sides; f.side_sums = a->side_sums; f.img_sums = a->img_sums; f.dsig = a->dsig;
  f.im_pose = im_pose; f.focal_log = focal_log; f.pp_raw = pp_raw; f.pw_pose = pw_pose;
  f.Mt = a->Mt; f.cam = a->cam;
  return f;
}

StepArgs step_args(const Align* a, float* depth_log) {
  StepArgs s;
  memset(&s, 0, sizeof(s));
  s.n = a->H * a->W; s.W = a->W; s.nwg = a->nwg;
  s.inv_En = (float)(1.0 / ((double)a->E * (double)a->H * (double)a->W));
  s.recs = a->recs; s.side_tab = a->side_tab; s.side_first = a->side_first; s.Mt = a->Mt; s.cam = a->cam;
  s.depth_log = depth_log; s.img_part = a->img_part; s.side_part = a->side_part;
  return s;
}

// one iteration's three launches (or, with f.loss_out null, the prepare launch alone)
int launch_iteration(const Align* a, hipStream_t stream, const StepArgs& s, const FinishArgs& f) {
  if (f.loss_out) {
    GS_KRANGE("align_step");
    hipLaunchKernelGGL(k_align_step, dim3(a->nwg, a->V), dim3(256), 0, stream, s);
    GS_CHECK_LAUNCH("align_step");
    GS_KRANGE("align_reduce");
    hipLaunchKernelGGL(k_align_reduce, dim3(2 * a->E + a->V), dim3(256), 0, stream, 2 * a->E, a->nwg, (const float*)a->side_part,
                       (const float*)a->img_part, a->side_sums, a->img_sums);
    GS_CHECK_LAUNCH("align_reduce");
  }
  GS_KRANGE("align_finish");
  hipLaunchKernelGGL(k_align_finish, dim3(1), dim3(FINISH_THREADS), 0, stream, f);
  GS_CHECK_LAUNCH("align_finish");
  return MI355GS_OK;
}

}  // namespace

extern "C" {

size_t mi355gs_align_workspace_bytes(int V, int H, int W, int E, int flags) {
  if (!align_size_ok(V, H, W, E, flags)) return 0;
  Align a;
  memset(&a, 0, sizeof(a));
  a.V = V; a.H = H; a.W = W; a.E = E; a.flags = flags;
  a.nwg = (int)(((long long)H * W + ALIGN_BLOCK - 1) / ALIGN_BLOCK);
  return carve(a, nullptr);
}

void* mi355gs_align_create(void* workspace, int V, int H, int W, const int32_t* edges, int E, int flags, float base_scale) {
  if (!workspace || !edges || !align_size_ok(V, H, W, E, flags) || !(base_scale > 0.f)) return nullptr;
  uint32_t count[MAX_VIEWS] = {0};
  for (int e = 0; e < E; ++e) {
    const int i = edges[2 * e], j = edges[2 * e + 1];
    if (i < 0 || i >= V || j < 0 || j >= V || i == j) return nullptr;
    ++count[i]; ++count[j];
  }
  for (int v = 0; v < V; ++v)
    if (!count[v]) return nullptr;   // an image that no edge covers
  Align* a = (Align*)calloc(1, sizeof(Align));
  if (!a) return nullptr;
  a->V = V; a->H = H; a->W = W; a->E = E; a->flags = flags; a->base_scale = base_scale;
  a->nwg = (int)(((long long)H * W + ALIGN_BLOCK - 1) / ALIGN_BLOCK);
  a->h_side_tab = (uint32_t*)malloc(2 * (size_t)E * 4);
  a->h_side_first = (uint32_t*)malloc(((size_t)V + 1) * 4);
  a->h_edge_sides = (uint32_t*)malloc(2 * (size_t)E * 4);
  if (!a->h_side_tab || !a->h_side_first || !a->h_edge_sides) {
    free(a->h_side_tab); free(a->h_side_first); free(a->h_edge_sides); free(a);
    return nullptr;
  }
  // the edge sides grouped by image, in edge order inside an image
  uint32_t cursor[MAX_VIEWS];
  a->h_side_first[0] = 0;
  for (int v = 0; v < V; ++v) { cursor[v] = a->h_side_first[v]; a->h_side_first[v + 1] = a->h_side_first[v] + count[v]; }
  for (int e = 0; e < E; ++e)
    for (int side = 0; side < 2; ++side) {
      const uint32_t at = cursor[edges[2 * e + side]]++;
      a->h_side_tab[at] = 2u * (uint32_t)e + (uint32_t)side;
      a->h_edge_sides[2 * e + side] = at;
    }
  carve(*a, workspace);
  return a;
}

void mi355gs_align_destroy(void* handle) {
  Align* a = (Align*)handle;
  if (!a) return;
  free(a->h_side_tab); free(a->h_side_first); free(a->h_edge_sides); free(a);
}

int mi355gs_align_pack(void* handle, void* stream_, const float* pred_i, const float* pred_j, const float* conf_i, const float* conf_j) {
  GS_RANGE();
  Align* a = (Align*)handle;
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !pred_i || !pred_j || !conf_i || !conf_j) return MI355GS_EINVAL;
  int rc;
  if ((rc = upload_tables(a, stream))) return rc;
  const int n = a->H * a->W;
  GS_KRANGE("align_pack");
  hipLaunchKernelGGL(k_align_pack, dim3((unsigned)((n + 255) / 256), (unsigned)(2 * a->E)), dim3(256), 0, stream, n, pred_i, pred_j, conf_i,
                     conf_j, a->recs);
  GS_CHECK_LAUNCH("align_pack");
  return MI355GS_OK;
}

int mi355gs_align_grad(void* handle, void* stream_, const float* depth_log, const float* im_pose, const float* focal_log, const float* pp_raw,
                       const float* pw_pose, float* g_depth_log, float* g_im_pose, float* g_focal_log, float* g_pw_pose, float* loss) {
  GS_RANGE();
  Align* a = (Align*)handle;
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !depth_log || !im_pose || !focal_log || !pp_raw || !pw_pose || !g_depth_log || !g_im_pose || !g_focal_log || !g_pw_pose || !loss)
    return MI355GS_EINVAL;
  int rc;
  if ((rc = upload_tables(a, stream))) return rc;
  // nothing is written through the state pointers here: no schedule row means no update
  FinishArgs f = finish_args(a, (float*)im_pose, (float*)focal_log, pp_raw, (float*)pw_pose);
  StepArgs s = step_args(a, (float*)depth_log);
  if ((rc = launch_iteration(a, stream, s, f))) return rc;   // prepare: the tables
  s.g_depth = g_depth_log;
  f.g_im_pose = g_im_pose; f.g_focal = g_focal_log; f.g_pw_pose = g_pw_pose; f.loss_out = loss;
  return launch_iteration(a, stream, s, f);
}

int mi355gs_align_run(void* handle, void* stream_, int niter, const float* step_table, float* depth_log, float* im_pose, float* focal_log,
                      const float* pp_raw, float* pw_pose, float* m_depth_log, float* v_depth_log, float* m_im_pose, float* v_im_pose,
                      float* m_focal_log, float* v_focal_log, float* m_pw_pose, float* v_pw_pose, float* losses) {
  GS_RANGE();
  Align* a = (Align*)handle;
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || niter < 0 || !depth_log || !im_pose || !focal_log || !pp_raw || !pw_pose || !m_depth_log || !v_depth_log || !m_im_pose ||
      !v_im_pose || !m_focal_log || !v_focal_log || !m_pw_pose || !v_pw_pose)
    return MI355GS_EINVAL;
  if (niter == 0) return MI355GS_OK;
  if (!step_table || !losses) return MI355GS_EINVAL;
  int rc;
  if ((rc = upload_tables(a, stream))) return rc;
  FinishArgs f = finish_args(a, im_pose, focal_log, pp_raw, pw_pose);
  StepArgs s = step_args(a, depth_log);
  if ((rc = launch_iteration(a, stream, s, f))) return rc;   // prepare: the tables of iteration 0
  s.opt_depth = (a->flags & MI355GS_ALIGN_OPT_DEPTH) ? 1u : 0u;
  s.m_depth = m_depth_log; s.v_depth = v_depth_log;
  f.m_im_pose = m_im_pose; f.v_im_pose = v_im_pose; f.m_focal = m_focal_log; f.v_focal = v_focal_log;
  f.m_pw_pose = m_pw_pose; f.v_pw_pose = v_pw_pose;
  for (int k = 0; k < niter; ++k) {
    s.sched = f.sched = (const float4*)step_table + k;
    f.loss_out = losses + k;
    if ((rc = launch_iteration(a, stream, s, f))) return rc;
  }
  return MI355GS_OK;
}

int mi355gs_align_points(void* handle, void* stream_, const float* depth_log, const float* im_pose, const float* focal_log,
                         const float* pp_raw, const float* pw_pose, float* pts3d, float* depth) {
  GS_RANGE();
  Align* a = (Align*)handle;
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !depth_log || !im_pose || !focal_log || !pp_raw || !pw_pose || !pts3d || !depth) return MI355GS_EINVAL;
  int rc;
  if ((rc = upload_tables(a, stream))) return rc;
  const FinishArgs f = finish_args(a, (float*)im_pose, (float*)focal_log, pp_raw, (float*)pw_pose);
  if ((rc = launch_iteration(a, stream, step_args(a, (float*)depth_log), f))) return rc;   // prepare
  const int n = a->H * a->W;
  GS_KRANGE("align_points");
  hipLaunchKernelGGL(k_align_points, dim3((unsigned)((n + 255) / 256), (unsigned)a->V), dim3(256), 0, stream, n, a->W, (const float*)a->cam,
                     depth_log, pts3d, depth);
  GS_CHECK_LAUNCH("align_points");
  return MI355GS_OK;
}

const float* mi355gs_align_records(void* handle) {   // what align_init.hip's batches read as their sources
  return handle ? (const float*)((Align*)handle)->recs : nullptr;
}

}  // extern "C"
