// extern "C" entry points of libmi355gs.so (declared in include/mi355gs.h).
// Host-side only: argument checks, scratch-layout arithmetic, kernel enqueue order.
#include <stdio.h>
#include "common.h"
#include <dlfcn.h>
#include <cstdlib>

// ---- optional per-kernel timing (HIP events on the launch stream)
namespace {
constexpr int PROF_KINDS = 6, PROF_MAX = 8192;   // include/mi355gs.h, mi355gs_profile_read: composite forward / backward / render-only
                                                 // forward, fused L1+SSIM loss pass, per-tile sort, per-tile count
struct ProfState {
  bool on = false;
  unsigned long long* work_counters = nullptr;   // device uint64[16] or null (mi355gs_profile_work_counters)
  hipEvent_t ev[PROF_KINDS][PROF_MAX][2];
  int created[PROF_KINDS] = {};
  int used[PROF_KINDS] = {};
  int period = 1;                   // events go around every period-th launch of a kind (mi355gs_profile_set_period)
  int seen[PROF_KINDS] = {};       // launches of the kind since profile_begin
} g_prof;
}  // namespace

GsProfScope::GsProfScope(int kind, hipStream_t stream) : s(stream) {
  if (!g_prof.on || kind < 0 || kind >= PROF_KINDS || g_prof.used[kind] >= PROF_MAX) return;
  if (g_prof.seen[kind]++ % g_prof.period != 0) return;
  const int i = g_prof.used[kind];
  if (i >= g_prof.created[kind]) {
    if (hipEventCreate(&g_prof.ev[kind][i][0]) != hipSuccess || hipEventCreate(&g_prof.ev[kind][i][1]) != hipSuccess) return;
    g_prof.created[kind] = i + 1;
  }
  (void)hipEventRecord(g_prof.ev[kind][i][0], s);
  stop = g_prof.ev[kind][i][1];
  g_prof.used[kind] = i + 1;
  active = true;
}
GsProfScope::~GsProfScope() { if (active) (void)hipEventRecord(stop, s); }
typedef GsProfScope ProfScope;

// ---- roctx ranges (mi355gs_profile_ranges): the marker library is opened at run time, on request
bool g_ranges_on = false;
thread_local bool g_krange_open = false;
namespace {
struct Roctx {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
  bool tried = false;
  unsigned long long pushed = 0;
} g_roctx;
bool roctx_open() {
  if (!g_roctx.tried) {
    g_roctx.tried = true;
    for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
      void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (!h) continue;
      g_roctx.push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
      g_roctx.pop = (int (*)())dlsym(h, "roctxRangePop");
      if (g_roctx.push && g_roctx.pop) break;
      g_roctx.push = nullptr; g_roctx.pop = nullptr;
    }
  }
  return g_roctx.push != nullptr;
}
struct RoctxEnv {   // MI355GS_ROCTX=1: ranges from the first call on (a whole run under rocprofv3 --marker-trace)
  RoctxEnv() { const char* e = getenv("MI355GS_ROCTX"); if (e && e[0] == '1' && roctx_open()) g_ranges_on = true; }
} g_roctx_env;
}  // namespace
void gs_range_push(const char* name) { ++g_roctx.pushed; (void)g_roctx.push(name); }
void gs_range_pop() { (void)g_roctx.pop(); }

void gs_log_error(const char* where, const char* what) { fprintf(stderr, "[mi355gs] %s failed: %s\n", where, what); }

static int g_scale_grad_exact = 0;   // mi355gs_tune_scale_grad
static int g_deterministic = 0;      // mi355gs_tune_deterministic
GsKnobs gs_knobs() { return GsKnobs{gs_min_units(), g_deterministic}; }

static CamParams make_cam(const float* view, const float* proj, const float* campos, float tanfovx, float tanfovy,
                          float scale_modifier, int W, int H) {
  CamParams cp;
  cp.view = view; cp.proj = proj; cp.campos = campos;
  cp.tanfovx = tanfovx; cp.tanfovy = tanfovy;
  cp.focal_x = W / (2.0f * tanfovx); cp.focal_y = H / (2.0f * tanfovy);
  cp.scale_modifier = scale_modifier;
  cp.scale_grad_factor = g_scale_grad_exact ? scale_modifier : 1.0f;
  cp.W = W; cp.H = H;
  cp.gx = (W + GS_TILE - 1) / GS_TILE; cp.gy = (H + GS_TILE - 1) / GS_TILE;
  return cp;
}

// the handles' device constants (common.h)
namespace {
__global__ void k_view_consts(float* consts) {
  const int i = threadIdx.x;
  if (i < 16) consts[i] = (i % 5 == 0) ? 1.f : 0.f;  // identity view matrix
  else if (i < 19) consts[i] = 0.f;                   // camera position
}
}  // namespace
int gs_write_view_consts(hipStream_t stream, float* consts, const char* name) {
  GS_KRANGE(name);
  hipLaunchKernelGGL(k_view_consts, dim3(1), dim3(64), 0, stream, consts);
  GS_CHECK_LAUNCH(name);
  return MI355GS_OK;
}

// ---- one frame, explicitly (common.h): the bodies of the public mi355gs_raster_* operators below.  Each validates what it is
// handed, so that mi355gs_posed_* and the handles answer a bad argument as the operators do, and opens the range the operator
// is known by in a marker trace.

int gs_frame_project(hipStream_t stream, const GsScene& sc, const GsView& vw, const GsFrameBufs& fb, const GsFrameCtx& cx,
                     int32_t* num_rendered, uint8_t* visible, int debug) {
  GsRange range("mi355gs_raster_forward_preprocess");
  const int P = sc.P, D = sc.D, M = sc.M, W = vw.W, H = vw.H;
  if (P < 0 || !gs_frame_size_ok(W, H) || D < 0 || D > 3) return MI355GS_EINVAL;
  if (!fb.geom || !fb.tiles || !num_rendered || !vw.view || !vw.proj || !vw.campos) return MI355GS_EINVAL;
  if (P > 0 && (!sc.means3D || !sc.opacities || !fb.radii)) return MI355GS_EINVAL;
  if (P > 0 && ((sc.shs == nullptr) == (sc.colors_precomp == nullptr))) return MI355GS_EINVAL;
  if (P > 0 && sc.shs && M < (D + 1) * (D + 1)) return MI355GS_EINVAL;
  if (sc.shs_rest && (!sc.shs || M < 2)) return MI355GS_EINVAL;
  if (P > 0 && !sc.cov3D_precomp && (!sc.scales || !sc.rotations)) return MI355GS_EINVAL;
  const GsFrame f({fb.geom, fb.tiles, nullptr, 0, fb.radii, fb.grad_scratch, fb.knobs}, P, W, H);   // no stage-1 kernel touches `binning`
  // The frame's accumulators are cleared by the projection kernel on its way (a fused caller hands over its own list): the
  // per-tile count + cursor words (adjacent), and — if the caller already holds the buffer its backward will use — the moment
  // records with the gate flags behind them.  No Gaussians, no kernel: memsets then.
  GsPrologue pro;
  if (cx.prologue) {
    pro = *cx.prologue;
  } else {
    pro.tile_counters = f.count; pro.n_counters = f.n_counters;
    if (fb.grad_scratch) { pro.grad_records = (float4*)fb.grad_scratch; pro.n_vec = gs_grad_gate_offset(P) / 16 + 2; }
    if (P <= 0) {
      if (hipMemsetAsync(f.count, 0, (size_t)f.n_counters * 4, stream) != hipSuccess) return MI355GS_ELAUNCH;
      if (fb.grad_scratch && hipMemsetAsync(fb.grad_scratch, 0, gs_grad_gate_offset(P) + 32, stream) != hipSuccess) return MI355GS_ELAUNCH;
    }
  }
  const CamParams cp = make_cam(vw.view, vw.proj, vw.campos, vw.tanfovx, vw.tanfovy, sc.scale_modifier, W, H);
  GS_KRANGE("preprocess_fwd");
  gs_launch_preprocess_fwd(stream, sc, cp, f, visible, cx.posed, pro);
  GS_CHECK_LAUNCH_SYNC("preprocess_fwd", stream, debug);
  GS_KRANGE("count_tiles");
  gs_launch_count_tiles(stream, f);
  GS_CHECK_LAUNCH_SYNC("count_tiles", stream, debug);
  GS_KRANGE("scan_tiles");
  gs_launch_scan_tiles(stream, f, num_rendered, fb.knobs.min_units);
  GS_CHECK_LAUNCH_SYNC("scan_tiles", stream, debug);
  return MI355GS_OK;
}

// Stage 2 of the forward in its two forms: `train` leaves the backward's work units, boundary records, hit masks and quadrant
// maxima in `binning` / `tiles`; render-only has a `binning` of keys + lists only and writes the image and the per-pixel state.
int gs_frame_render(hipStream_t stream, int P, const GsView& vw, const GsFrameBufs& fb, const float* bg, float* out_color, bool train,
                    int debug) {
  GsRange range(train ? "mi355gs_raster_forward_render" : "mi355gs_raster_forward_render_only");
  const int W = vw.W, H = vw.H;
  if (P < 0 || W <= 0 || H <= 0 || !fb.geom || !fb.tiles || !bg || !out_color) return MI355GS_EINVAL;
  if (clamp_capacity(fb.capacity) > 0 && !fb.binning) return MI355GS_EINVAL;
  const GsFrame f(fb, P, W, H);
  GS_KRANGE("binning");
  gs_launch_binning(stream, f);
  GS_CHECK_LAUNCH_SYNC("binning", stream, debug);
  {
    ProfScope prof(train ? 0 : 2, stream);
    GS_KRANGE("composite_fwd");
    gs_launch_composite_fwd(stream, f, bg, out_color, train ? g_prof.work_counters : nullptr, train);
  }
  GS_CHECK_LAUNCH_SYNC("composite_fwd", stream, debug);
  return MI355GS_OK;
}

int gs_frame_backward(hipStream_t stream, const GsScene& sc, const GsView& vw, const GsFrameBufs& fb, const GsFrameCtx& cx,
                      const float* bg, const float* out_color, const float* dL_dpix, const GsGradOut& o, bool grad_scratch_is_clear,
                      int debug) {
  GsRange range("mi355gs_raster_backward");
  const int P = sc.P, D = sc.D, W = vw.W, H = vw.H;
  if (P < 0 || W <= 0 || H <= 0 || D < 0 || D > 3) return MI355GS_EINVAL;
  if (!fb.geom || !fb.tiles || !dL_dpix || !out_color || !fb.grad_scratch || !bg || !vw.view || !vw.proj || !vw.campos) return MI355GS_EINVAL;
  const bool outs = !(cx.pose_only && cx.posed.pose);   // pose-only stores no output, so none is required
  if (P > 0 && (!sc.means3D || !fb.radii || (outs && (!o.means3D || !o.means2D || !o.opacities)))) return MI355GS_EINVAL;
  const int use_shs = sc.shs != nullptr, use_cov = sc.cov3D_precomp != nullptr;
  if (P > 0 && outs && use_shs && !o.shs) return MI355GS_EINVAL;
  if (sc.shs_rest && !use_shs) return MI355GS_EINVAL;
  if (P > 0 && outs && !use_shs && !o.colors) return MI355GS_EINVAL;
  if (P > 0 && !use_cov && (!sc.scales || !sc.rotations || (outs && (!o.scales || !o.rotations)))) return MI355GS_EINVAL;
  if (P > 0 && outs && use_cov && !o.cov3D) return MI355GS_EINVAL;
  if (P == 0) return MI355GS_OK;
  if (clamp_capacity(fb.capacity) > 0 && !fb.binning) return MI355GS_EINVAL;
  const GsFrame f(fb, P, W, H);
  GsGrad* grads = (GsGrad*)fb.grad_scratch;
  // (with gate_tail the eight gate flags behind the records are cleared by the same memset)
  const size_t clear_bytes = cx.gate_tail ? gs_grad_gate_offset(P) + 8 * sizeof(float) : (size_t)P * sizeof(GsGrad);
  if (!cx.prologue && !grad_scratch_is_clear && hipMemsetAsync(grads, 0, clear_bytes, stream) != hipSuccess) return MI355GS_ELAUNCH;
  if (f.cap > 0) {
    // deterministic mode: every instance's moments go to a row of their own (binning: det_rows / det_rowidx) and are summed per
    // Gaussian in rectangle order by k_det_gather, which writes every record — instead of meeting in float atomics
    const bool det = fb.knobs.det != 0;
    char* det_scratch = (char*)fb.grad_scratch + gs_grad_gate_offset(P) + 256;
    if (det) {
      GS_KRANGE("det_prepare");
      const int rc = gs_launch_det_prepare(stream, f, det_scratch);
      GS_CHECK_LAUNCH_SYNC("det_prepare", stream, debug);
      if (rc != 0) return MI355GS_ELAUNCH;
    }
    {
      ProfScope prof(1, stream);
      GS_KRANGE("composite_bwd");
      gs_launch_composite_bwd(stream, f, bg, dL_dpix, grads, out_color, det ? nullptr : g_prof.work_counters);
    }
    GS_CHECK_LAUNCH_SYNC("composite_bwd", stream, debug);
    if (det) {
      GS_KRANGE("det_gather");
      gs_launch_det_gather(stream, f, det_scratch, grads);
      GS_CHECK_LAUNCH_SYNC("det_gather", stream, debug);
    }
  }
  const CamParams cp = make_cam(vw.view, vw.proj, vw.campos, vw.tanfovx, vw.tanfovy, sc.scale_modifier, W, H);
  GS_KRANGE("preprocess_bwd");
  gs_launch_preprocess_bwd(stream, sc, cp, f, grads, o, cx.posed, cx.gate, cx.pose_only);
  GS_CHECK_LAUNCH_SYNC("preprocess_bwd", stream, debug);
  return MI355GS_OK;
}

extern "C" {

int mi355gs_abi_version(void) { return MI355GS_ABI_VERSION; }

const char* mi355gs_error_string(int code) {
  switch (code) {
    case MI355GS_OK: return "ok";
    case MI355GS_EINVAL: return "invalid argument";
    case MI355GS_ELAUNCH: return "HIP launch or runtime failure";
    case MI355GS_EOVERFLOW: return "instance capacity exceeded";
    default: return "unknown error";
  }
}

// the size queries answer for the knobs as they stand now
size_t mi355gs_raster_geom_bytes(int P) { return GeomLayout(P).total; }
size_t mi355gs_raster_tiles_bytes(int W, int H) { return (W > 0 && H > 0) ? TilesLayout(W, H).total : 0; }
size_t mi355gs_raster_binning_bytes(int64_t n, int W, int H) { return (W > 0 && H > 0) ? gs_binning_bytes(n, W, H, gs_knobs(), true) : 0; }
size_t mi355gs_raster_binning_bytes_render_only(int64_t n, int W, int H) { return (W > 0 && H > 0) ? gs_binning_bytes(n, W, H, gs_knobs(), false) : 0; }
size_t mi355gs_raster_grad_gate_offset(int P) { return gs_grad_gate_offset(P); }
size_t mi355gs_raster_grad_scratch_bytes(int P) { return gs_grad_scratch_bytes(P, g_deterministic); }

// ---- the stateless operators: the frame functions with the current knobs and no context
int mi355gs_raster_forward_preprocess(void* stream, int P, int D, int M, int W, int H, const float* means3D, const float* shs,
                                      const float* shs_rest, const float* colors_precomp, const float* opacities, const float* scales,
                                      float scale_modifier, const float* rotations, const float* cov3D_precomp,
                                      const float* viewmatrix, const float* projmatrix, const float* campos, float tanfovx,
                                      float tanfovy, int prefiltered, int32_t* radii, void* geom, void* tiles,
                                      int32_t* num_rendered, uint8_t* visible, void* grad_scratch, int debug) {
  (void)prefiltered;  // as in the reference operator it only affects an internal consistency check
  return gs_frame_project((hipStream_t)stream, {P, D, M, means3D, shs, shs_rest, colors_precomp, opacities, scales, rotations, cov3D_precomp, scale_modifier},
                          {W, H, viewmatrix, projmatrix, campos, tanfovx, tanfovy}, {geom, tiles, nullptr, 0, radii, grad_scratch, gs_knobs()},
                          GsFrameCtx(), num_rendered, visible, debug);
}

int mi355gs_raster_forward_render(void* stream, int P, int W, int H, int64_t capacity, const float* bg, const void* geom,
                                  void* tiles, void* binning, float* out_color, int debug) {
  return gs_frame_render((hipStream_t)stream, P, {W, H}, {const_cast<void*>(geom), tiles, binning, capacity, nullptr, nullptr, gs_knobs()}, bg,
                         out_color, true, debug);
}

int mi355gs_raster_forward_render_only(void* stream, int P, int W, int H, int64_t capacity, const float* bg, const void* geom,
                                       void* tiles, void* binning, float* out_color, int debug) {
  return gs_frame_render((hipStream_t)stream, P, {W, H}, {const_cast<void*>(geom), tiles, binning, capacity, nullptr, nullptr, gs_knobs()}, bg,
                         out_color, false, debug);
}

int mi355gs_raster_backward(void* stream, int P, int D, int M, int W, int H, const float* bg, const float* means3D,
                            const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities, const float* scales,
                            float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                            const float* projmatrix, const float* campos, float tanfovx, float tanfovy, const void* geom,
                            void* tiles, const void* binning, int64_t capacity, const int32_t* radii, const float* out_color,
                            const float* dL_dpix, void* grad_scratch, float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs,
                            float* dL_dshs_rest, float* dL_dcolors, float* dL_dopacities, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
                            int grad_scratch_is_clear, int debug) {
  const GsGradOut o = {dL_dmeans3D, dL_dmeans2D, dL_dshs, dL_dshs_rest, dL_dcolors, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D};
  return gs_frame_backward((hipStream_t)stream, {P, D, M, means3D, shs, shs_rest, colors_precomp, opacities, scales, rotations, cov3D_precomp, scale_modifier},
                           {W, H, viewmatrix, projmatrix, campos, tanfovx, tanfovy},
                           {const_cast<void*>(geom), tiles, const_cast<void*>(binning), capacity, const_cast<int32_t*>(radii), grad_scratch, gs_knobs()},
                           GsFrameCtx(), bg, out_color, dL_dpix, o, grad_scratch_is_clear != 0, debug);
}

// ---- depth and accumulated-alpha maps: a pass over the frame's lists beside the colour kernels (composite.hip), and its backward
namespace {
struct DepthScratchLayout {   // the depth backward's own accumulators: moment records (colour slots stay zero), dL/dz per Gaussian
  size_t grads, dz, total;
  explicit DepthScratchLayout(int P) {
    const size_t n = P > 0 ? (size_t)P : 1;
    size_t o = 0;
    grads = o; o += gs_align(n * sizeof(GsGrad));
    dz = o; o += gs_align(n * sizeof(float));
    total = o;
  }
};
}  // namespace

size_t mi355gs_raster_depth_scratch_bytes(int P) { return DepthScratchLayout(P).total; }

int mi355gs_raster_depth_forward(void* stream_, int P, int W, int H, int64_t capacity, const void* geom, const void* tiles,
                                 const void* binning, float* out_depth, float* out_alpha) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (P < 0 || !gs_frame_size_ok(W, H) || !geom || !tiles) return MI355GS_EINVAL;
  const uint32_t cap = clamp_capacity(capacity);
  if (cap > 0 && !binning) return MI355GS_EINVAL;
  const size_t map_bytes = (size_t)W * H * sizeof(float);
  if (P == 0 || cap == 0) {   // nothing blends anywhere
    if (out_depth && hipMemsetAsync(out_depth, 0, map_bytes, stream) != hipSuccess) return MI355GS_ELAUNCH;
    if (out_alpha && hipMemsetAsync(out_alpha, 0, map_bytes, stream) != hipSuccess) return MI355GS_ELAUNCH;
    return MI355GS_OK;
  }
  if (!out_depth && !out_alpha) return MI355GS_OK;
  // (the list's offset does not depend on the knobs)
  const GsFrame f({const_cast<void*>(geom), const_cast<void*>(tiles), const_cast<void*>(binning), capacity, nullptr, nullptr, gs_knobs()}, P, W, H);
  GS_KRANGE("depth_fwd");
  gs_launch_depth_fwd(stream, f, out_depth, out_alpha);
  GS_CHECK_LAUNCH("depth_fwd");
  return MI355GS_OK;
}

int mi355gs_raster_depth_backward(void* stream_, int P, int W, int H, const float* means3D, const float* scales, float scale_modifier,
                                  const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                                  const float* campos, float tanfovx, float tanfovy, const void* geom, const void* tiles, const void* binning,
                                  int64_t capacity, const int32_t* radii, const float* dL_ddepth, const float* dL_dalpha, void* depth_scratch,
                                  float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacities, float* dL_dscales, float* dL_drotations,
                                  float* dL_dcov3D, int debug) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (P < 0 || !gs_frame_size_ok(W, H)) return MI355GS_EINVAL;
  if (!geom || !tiles || !depth_scratch || !viewmatrix || !projmatrix || !campos) return MI355GS_EINVAL;
  const int use_cov = cov3D_precomp != nullptr;
  if (P > 0 && (!means3D || !radii || !dL_dmeans3D || !dL_dmeans2D || !dL_dopacities)) return MI355GS_EINVAL;
  if (P > 0 && !use_cov && (!scales || !rotations || !dL_dscales || !dL_drotations)) return MI355GS_EINVAL;
  if (P > 0 && use_cov && !dL_dcov3D) return MI355GS_EINVAL;
  const uint32_t cap = clamp_capacity(capacity);
  if (cap > 0 && !binning) return MI355GS_EINVAL;
  if (P == 0) return MI355GS_OK;
  const GsFrame f({const_cast<void*>(geom), const_cast<void*>(tiles), const_cast<void*>(binning), capacity, const_cast<int32_t*>(radii),
                   nullptr, gs_knobs()}, P, W, H);
  const DepthScratchLayout dl(P);
  GsGrad* grads = (GsGrad*)((char*)depth_scratch + dl.grads);
  float* dz = (float*)((char*)depth_scratch + dl.dz);
  if (hipMemsetAsync(depth_scratch, 0, dl.total, stream) != hipSuccess) return MI355GS_ELAUNCH;
  if (f.cap > 0 && (dL_ddepth || dL_dalpha)) {
    GS_KRANGE("depth_bwd");
    gs_launch_depth_bwd(stream, f, dL_ddepth, dL_dalpha, grads, dz);
    GS_CHECK_LAUNCH_SYNC("depth_bwd", stream, debug);
  }
  // the moments -> dL/dmean2D, dL/dconic, dL/dopacity -> means, scales, rotations / cov3D: the projection backward over a scene
  // without colours.  The colour slots of the records are zero, so nothing colour-borne exists: no dL_dcolors is stored.
  const GsScene sc = {P, 0, 0, means3D, nullptr, nullptr, nullptr, nullptr, scales, rotations, cov3D_precomp, scale_modifier};
  const GsGradOut o = {dL_dmeans3D, dL_dmeans2D, nullptr, nullptr, nullptr, dL_dopacities, dL_dscales, dL_drotations, dL_dcov3D};
  const CamParams cp = make_cam(viewmatrix, projmatrix, campos, tanfovx, tanfovy, scale_modifier, W, H);
  GS_KRANGE("preprocess_bwd");
  gs_launch_preprocess_bwd(stream, sc, cp, f, grads, o, GsPosed(), nullptr, false);
  GS_CHECK_LAUNCH_SYNC("preprocess_bwd", stream, debug);
  GS_KRANGE("depth_dz");
  gs_launch_depth_dz(stream, P, viewmatrix, dz, dL_dmeans3D);
  GS_CHECK_LAUNCH_SYNC("depth_dz", stream, debug);
  return MI355GS_OK;
}

int mi355gs_tune_deterministic(int on) {
  const int old = g_deterministic;
  if (on >= 0) g_deterministic = on ? 1 : 0;
  return old;
}

int mi355gs_tune_scale_grad(int mode) {
  const int old = g_scale_grad_exact;
  if (mode >= 0) g_scale_grad_exact = mode ? 1 : 0;
  return old;
}

int mi355gs_raster_frame_stats(void* stream_, int W, int H, const void* tiles, int64_t* stats) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (W <= 0 || H <= 0 || !tiles || !stats) return MI355GS_EINVAL;
  if (hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), stream) != hipSuccess) return MI355GS_ELAUNCH;
  const GsFrame f(const_cast<void*>(tiles), W, H);
  GS_KRANGE("frame_stats");
  gs_launch_frame_stats(stream, f, stats);
  GS_CHECK_LAUNCH("frame_stats");
  return MI355GS_OK;
}

int mi355gs_profile_begin(void) {
  g_prof.on = true;
  for (int k = 0; k < PROF_KINDS; ++k) g_prof.used[k] = g_prof.seen[k] = 0;
  return MI355GS_OK;
}

int mi355gs_profile_set_period(int every) {
  const int old = g_prof.period;
  if (every > 0) g_prof.period = every;
  return old;
}

int mi355gs_profile_work_counters(void* counters) {
  g_prof.work_counters = (unsigned long long*)counters;
  return MI355GS_OK;
}

int mi355gs_profile_read(int kind, double* total_ms, int* launches) {
  if (kind < 0 || kind >= PROF_KINDS || !total_ms || !launches) return MI355GS_EINVAL;
  double tot = 0.0;
  for (int i = 0; i < g_prof.used[kind]; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(g_prof.ev[kind][i][1]) != hipSuccess) return MI355GS_ELAUNCH;
    if (hipEventElapsedTime(&ms, g_prof.ev[kind][i][0], g_prof.ev[kind][i][1]) != hipSuccess) return MI355GS_ELAUNCH;
    tot += ms;
  }
  *total_ms = tot;
  *launches = g_prof.used[kind];
  return MI355GS_OK;
}

int mi355gs_profile_end(void) {
  g_prof.on = false;
  return MI355GS_OK;
}

int mi355gs_profile_ranges(int on) {
  if (on == 1) {
    if (!roctx_open()) return MI355GS_EINVAL;
    g_ranges_on = true;
  } else if (on == 0) {
    g_ranges_on = false;
  }
  return (int)(g_roctx.pushed & 0x7fffffffull);
}

int mi355gs_raster_mark_visible(void* stream_, int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                                uint8_t* present) {
  GS_RANGE();
  (void)projmatrix;
  if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) return MI355GS_EINVAL;
  GS_KRANGE("mark_visible");
  gs_launch_mark_visible((hipStream_t)stream_, P, means3D, viewmatrix, present);
  GS_CHECK_LAUNCH("mark_visible");
  return MI355GS_OK;
}

}  // extern "C"
