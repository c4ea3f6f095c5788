// Test-view pose tracking behind one library call per view (include/mi355gs.h, mi355gs_tracker_*): the body of reference
// render.py:124-159 (`render_set_optimize`) for one view, with the Gaussians frozen:
//
//   posed projection -> tile binning -> composite -> masked L1 value + gradient -> composite backward
//   -> pose-only projection backward (16 pose sums per workgroup) -> finish: d_pose, Adam on the 7-vector, keep-best
//
// 10 kernel dispatches per iteration (projection, tile count, tile scan, scatter, tile sort, composite, masked L1, composite
// backward, projection backward, finish; 12 in deterministic mode with det_prepare / det_gather around the composite backward), no host
// synchronisation and no allocation: every buffer lives in one caller-provided workspace, the optimizer state in a caller-owned
// device block.  The projection, binning and composite kernels are the ones render() and the one-call train step run, called
// through the same frame functions (common.h, gs_frame_*) with this loop's context: the pose and the rows for its sums, the
// frame's accumulators cleared by the projection, and the projection backward in its pose-only instantiation, which
// stores none of the ~250 B per Gaussian of raw-parameter gradients and gate flags that frozen Gaussians never read.
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "pose_math.h"

namespace {

constexpr int L1_PER_THREAD = 4;   // masked-L1 elements per thread: one workgroup covers 1024 consecutive pixels of the [3,H,W] image
constexpr int L1_BLOCK = 256 * L1_PER_THREAD;

int l1_nblocks(int W, int H) { return (int)((3LL * W * H + L1_BLOCK - 1) / L1_BLOCK); }

struct Tracker : GsFrozenScene {
  char* grad_scratch;
  float *dL_dimg, *loss_partial, *pose_partial;
  bool consts_ready;
  GsKnobs knobs;   // as they stood at create: the buffers were laid out for them
};

size_t carve(Tracker& t, void* workspace) {
  GsCarver c{(char*)workspace};
  t.GsFrozenScene::carve(c, t.knobs, true);
  t.grad_scratch = c.take<char>(gs_grad_scratch_bytes(t.P, t.knobs.det));
  t.dL_dimg = c.take<float>(3 * (size_t)t.W * t.H);
  t.loss_partial = c.take<float>(2 * (size_t)l1_nblocks(t.W, t.H));
  t.pose_partial = c.take<float>(16 * (((size_t)t.P + 255) / 256));
  return c.off;
}

// Masked L1 (reference utils/loss_utils.py:17-23 with mask = render > 0): per workgroup the partial sums of |r - gt| * m and of
// m, and per element dL/dimg WITHOUT the 1 / sum(m) factor — sgn(r - gt) * m, sgn(0) = 0, a NaN difference propagating as in
// torch.sgn.  The factor is applied to the seven pose gradients by k_tracker_finish (the chain is linear in dL/dimg).
__global__ __launch_bounds__(256) void k_masked_l1(int n, const float* __restrict__ img, const float* __restrict__ gt,
                                                   float* __restrict__ dL_dimg, float* __restrict__ partial) {
  __shared__ float s_red[4][2];
  float a = 0.f, b = 0.f;
  const int base = blockIdx.x * L1_BLOCK + threadIdx.x;
#pragma unroll
  for (int j = 0; j < L1_PER_THREAD; ++j) {
    const int idx = base + j * 256;
    if (idx < n) {
      const float r = img[idx], d = r - gt[idx];
      const float m = r > 0.f ? 1.f : 0.f;
      const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : d * 0.f);   // (d * 0: +-0 for a zero difference, NaN for a NaN)
      dL_dimg[idx] = sg * m;
      a += fabsf(d) * m;
      b += m;
    }
  }
  a = gs_wave_sum_row3(a); b = gs_wave_sum_row3(b);   // every lane is active: the totals land in lanes 48..63
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 63) { s_red[wave][0] = a; s_red[wave][1] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = (s_red[0][0] + s_red[1][0]) + (s_red[2][0] + s_red[3][0]);
    partial[2 * blockIdx.x + 1] = (s_red[0][1] + s_red[1][1]) + (s_red[2][1] + s_red[3][1]);
  }
}

// torch.optim.Adam as torch 2.10 runs it (_multi_tensor_adam, the foreach path of a device tensor): L2 weight decay folded
// into the gradient, lerp for the first moment, mul + addcmul for the second, denom = sqrt(v) / bc2_sqrt + eps,
// p += step_size * (m / denom) with step_size = -lr / bc1.  Every scalar torch hands over as a Python float is rounded to fp32
// once, as the foreach kernels do.
constexpr float ADAM_WD = (float)1e-4;
constexpr float ADAM_LERP_W = (float)(1.0 - 0.9);     // exp_avg.lerp_(grad, 1 - beta1): weight < 0.5, self + w * (end - self)
constexpr float ADAM_BETA2 = (float)0.999;
constexpr float ADAM_ONE_MINUS_BETA2 = (float)(1.0 - 0.999);
constexpr float ADAM_EPS = (float)1e-8;

// One element of that step.  Rounding as torch's device foreach kernels round (measured on the MI355X, element by element):
// fused multiply-adds for the weight decay, the lerp, addcmul (on the rounded g*g) and addcdiv (on the rounded m / denom),
// correctly rounded sqrt and division — written out so that no other contraction can creep in.
__device__ __forceinline__ float tracker_adam(float p, float d, float& m, float& v, float step_size, float bc2_sqrt) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const float gr = fmaf(ADAM_WD, p, d);
  m = fmaf(ADAM_LERP_W, gr - m, m);
  const float gg = gr * gr;
  v = fmaf(ADAM_ONE_MINUS_BETA2, gg, v * ADAM_BETA2);
  const float denom = sqrtf(v) / bc2_sqrt + ADAM_EPS;
  const float q = m / denom;
  return fmaf(step_size, q, p);
}

// Single workgroup, after the projection backward: deterministic tree sum of the pose partials (the order of
// k_pose_finish_partials), double sum of the loss partials, d_pose, Adam, keep-best (reference render.py:149-152: the loss of
// iteration i, taken at the pre-step pose, is compared with `<` against the best so far; a lower one makes the POST-step pose
// the candidate; a NaN never wins).  The overflow gate reads the frame's instance count (tile_start[T]).
__global__ __launch_bounds__(1024) void k_tracker_finish(const float* __restrict__ partial, int nrows, const float* __restrict__ loss_partial,
                                                         int loss_nblocks, const uint32_t* __restrict__ count, const uint32_t* __restrict__ qmax,
                                                         int nq, unsigned long long capacity,
                                                         const float4* __restrict__ sched, int iter, float* __restrict__ state,
                                                         float* __restrict__ pose_trace, float* __restrict__ loss_trace,
                                                         float* __restrict__ grad_trace) {
  __shared__ float s_sum[16][17];
  __shared__ float s_tot[16];
  __shared__ double s_la[16], s_lb[16];
  __shared__ uint32_t s_blended;
  const int k = threadIdx.x & 15, g = threadIdx.x >> 4;
  if (threadIdx.x == 0) s_blended = 0u;
  float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
  {
    int r = g;
    for (; r + 192 < nrows; r += 256) {
      v0 += partial[(size_t)r * 16 + k]; v1 += partial[(size_t)(r + 64) * 16 + k];
      v2 += partial[(size_t)(r + 128) * 16 + k]; v3 += partial[(size_t)(r + 192) * 16 + k];
    }
    for (; r < nrows; r += 64) v0 += partial[(size_t)r * 16 + k];
  }
  {
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < loss_nblocks; i += 1024) { a += (double)loss_partial[2 * i]; b += (double)loss_partial[2 * i + 1]; }
    a = gs_wave_sum_row3_f64(a); b = gs_wave_sum_row3_f64(b);
    if ((threadIdx.x & 63) == 63) { s_la[threadIdx.x >> 6] = a; s_lb[threadIdx.x >> 6] = b; }
  }
  const float wsum = gs_sum_rows((v0 + v1) + (v2 + v3));
  if ((threadIdx.x & 63) < 16) s_sum[threadIdx.x >> 6][k] = wsum;
  __syncthreads();
  // An all-masked frame (every m = 0) with binned instances: was any (pixel, Gaussian) pair blended?  The forward's per-quadrant
  // maxima of the per-pixel contributor counts say so (a non-zero count is a blended pair).  Every thread sees the same 16 sums
  // (m >= 0: their total is 0 iff each is), so the whole workgroup takes this branch or none.
  bool masked_out = true;
  for (int w = 0; w < 16; ++w) masked_out = masked_out && s_lb[w] == 0.0;
  if (masked_out && *count > 0u) {
    uint32_t any = 0u;
    for (int i = threadIdx.x; i < nq; i += 1024) any |= qmax[i];
    if (any) s_blended = 1u;
  }
  if (threadIdx.x < 16) {
    float t = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) t += s_sum[q][threadIdx.x];
    s_tot[threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double la = 0.0, lb = 0.0;
  for (int w = 0; w < 16; ++w) { la += s_la[w]; lb += s_lb[w]; }
  float total[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) total[c] = s_tot[c];
  float* pose = state + MI355GS_TRACKER_POSE;
  float d[7];
  pose_grad_from_sums(load_pose(pose), total, d);
  const uint32_t cnt = *count;
  // loss = sum(|r - gt| * m) / sum(m); the gradient's 1 / sum(m) in fp32 as autograd forms it.  An all-masked frame (sum(m) = 0):
  // autograd's dL/dimg is NaN at every pixel (0 * inf), which reaches the pose through every Gaussian the composite backward
  // touches — a blended one — and nothing when no pair was blended (no instance binned, or none passing the alpha test), where
  // its pose gradient is exactly zero.
  const float loss = (float)(la / lb);
  const float inv = lb > 0.0 ? 1.0f / (float)lb : (s_blended ? __int_as_float(0x7fc00000) : 0.0f);
#pragma unroll
  for (int c = 0; c < 7; ++c) d[c] = lb > 0.0 ? d[c] * inv : inv;
  if (pose_trace)
    for (int c = 0; c < 7; ++c) pose_trace[7 * (size_t)iter + c] = pose[c];
  if (loss_trace) loss_trace[iter] = loss;
  if (grad_trace)
    for (int c = 0; c < 7; ++c) grad_trace[7 * (size_t)iter + c] = d[c];
  uint32_t* flag = reinterpret_cast<uint32_t*>(state + MI355GS_TRACKER_FLAG);
  uint32_t* seen = reinterpret_cast<uint32_t*>(state + MI355GS_TRACKER_COUNT);
  if (cnt > *seen) *seen = cnt;
  if ((unsigned long long)cnt > capacity) *flag = 1u;
  if (*flag) return;   // sticky: this frame dropped instances, or an earlier one did — nothing after it is the view's trajectory
  if (iter == 0) state[MI355GS_TRACKER_INITIAL] = loss;
  const float4 s = sched[iter];   // (step_size t, step_size q, bc2_sqrt, -)
  float* m = state + MI355GS_TRACKER_EXP_AVG;
  float* v = state + MI355GS_TRACKER_EXP_AVG_SQ;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    float mc = m[c], vc = v[c];
    pose[c] = tracker_adam(pose[c], d[c], mc, vc, c < 4 ? s.y : s.x, s.z);
    m[c] = mc; v[c] = vc;
  }
  if (loss < state[MI355GS_TRACKER_BEST]) {
    state[MI355GS_TRACKER_BEST] = loss;
    for (int c = 0; c < 7; ++c) state[MI355GS_TRACKER_CAND + c] = pose[c];
  }
}

int ensure_consts(Tracker* t, hipStream_t stream) {   // written once, on the stream of the handle's first call
  if (t->consts_ready) return MI355GS_OK;
  const int rc = gs_write_view_consts(stream, t->consts, "tracker_consts");
  t->consts_ready = rc == MI355GS_OK;
  return rc;
}

}  // namespace

extern "C" {

size_t mi355gs_tracker_workspace_bytes(int P, int W, int H, int64_t capacity) {
  if (P <= 0 || W <= 0 || H <= 0 || capacity <= 0) return 0;
  Tracker t;
  memset(&t, 0, sizeof(t));
  t.P = P; t.W = W; t.H = H; t.capacity = capacity; t.knobs = gs_knobs();
  return carve(t, nullptr);
}

void* mi355gs_tracker_create(int P, int M, int W, int H, int64_t capacity, const float* xyz, const float* f_dc, const float* f_rest,
                             const float* opacity, const float* scaling, const float* rotation, void* workspace) {
  Tracker* t = (Tracker*)calloc(1, sizeof(Tracker));
  if (!t) return nullptr;
  if (!t->init(P, M, W, H, capacity, xyz, f_dc, f_rest, opacity, scaling, rotation, workspace)) { free(t); return nullptr; }
  t->knobs = gs_knobs();
  carve(*t, workspace);
  return t;
}

void mi355gs_tracker_destroy(void* handle) { free(handle); }

int mi355gs_tracker_count(void* handle, void* stream_, int sh_degree, const float* projmatrix, float tanfovx, float tanfovy,
                          const float* pose, int32_t* count_out) {
  GS_RANGE();
  Tracker* t = (Tracker*)handle;
  hipStream_t stream = (hipStream_t)stream_;
  if (!t || !t->degree_ok(sh_degree) || !projmatrix || !pose || !count_out) return MI355GS_EINVAL;
  int rc;
  if ((rc = ensure_consts(t, stream))) return rc;
  GsFrameCtx cx;
  cx.posed.pose = pose;
  return gs_frame_project(stream, t->scene(sh_degree), t->view(projmatrix, tanfovx, tanfovy), t->bufs(t->knobs, nullptr), cx, count_out,
                          nullptr, 0);
}

int mi355gs_tracker_run(void* handle, void* stream_, int sh_degree, const float* gt_image, const float* projmatrix, float tanfovx,
                        float tanfovy, const float* bg, const float* sched, int num_iter, int first_iter, int n_iters, float* state,
                        float* pose_trace, float* loss_trace, float* grad_trace) {
  GS_RANGE();
  Tracker* t = (Tracker*)handle;
  hipStream_t stream = (hipStream_t)stream_;
  if (!t || !t->degree_ok(sh_degree) || !gt_image || !projmatrix || !bg || !sched || !state) return MI355GS_EINVAL;
  if (num_iter <= 0 || first_iter < 0 || n_iters < 0 || first_iter > num_iter || n_iters > num_iter - first_iter) return MI355GS_EINVAL;
  if (n_iters == 0) return MI355GS_OK;
  int rc;
  if ((rc = ensure_consts(t, stream))) return rc;
  const int P = t->P, W = t->W, H = t->H;
  const int n_pix = 3 * W * H, l1_blocks = l1_nblocks(W, H), rows = (P + 255) / 256;
  const GsScene scene = t->scene(sh_degree);
  const GsView view = t->view(projmatrix, tanfovx, tanfovy);
  const GsFrameBufs bufs = t->bufs(t->knobs, t->grad_scratch);
  const GsFrame f(bufs, P, W, H);
  // the frame's accumulators (moment records, per-tile counters) are cleared by its first kernel, the projection
  GsPrologue pro;
  pro.grad_records = (float4*)t->grad_scratch; pro.n_vec = (size_t)P * 3;
  pro.tile_counters = f.count; pro.n_counters = f.n_counters;
  GsFrameCtx cx;
  cx.prologue = &pro;
  cx.posed.pose = state + MI355GS_TRACKER_POSE;
  cx.posed.acc = t->pose_partial;     // unused with `partial` set; kept valid
  cx.posed.partial = t->pose_partial; // one row of 16 pose sums per projection workgroup
  cx.pose_only = true;
  for (int it = first_iter; it < first_iter + n_iters; ++it) {
    if ((rc = gs_frame_project(stream, scene, view, bufs, cx, t->num_rendered, nullptr, 0))) return rc;
    if ((rc = gs_frame_render(stream, P, view, bufs, bg, t->image, true, 0))) return rc;
    GS_KRANGE("masked_l1");
    hipLaunchKernelGGL(k_masked_l1, dim3(l1_blocks), dim3(256), 0, stream, n_pix, t->image, gt_image, t->dL_dimg, t->loss_partial);
    GS_CHECK_LAUNCH("masked_l1");
    if ((rc = gs_frame_backward(stream, scene, view, bufs, cx, bg, t->image, t->dL_dimg, GsGradOut(), false, 0))) return rc;
    GS_KRANGE("tracker_finish");
    hipLaunchKernelGGL(k_tracker_finish, dim3(1), dim3(1024), 0, stream, (const float*)t->pose_partial, rows,
                       (const float*)t->loss_partial, l1_blocks, t->count(), f.qmax, 4 * f.T,
                       (unsigned long long)t->capacity, (const float4*)sched, it, state,
                       pose_trace, loss_trace, grad_trace);
    GS_CHECK_LAUNCH("tracker_finish");
  }
  return MI355GS_OK;
}

}  // extern "C"
