// Camera paths behind one library call (include/mi355gs.h, mi355gs_path_* and mi355gs_rgb8_from_planar): the body of reference
// render.py:85-93 (`render_set`) for a list of poses, with the Gaussians frozen and nothing to differentiate:
//
//   posed projection -> tile binning -> render-only composite -> 8-bit interleaved frame (+ the frame's instance count)
//
// 7 kernel dispatches per frame (projection, tile count, tile scan, scatter, tile sort, composite, 8-bit conversion), no host
// synchronisation, no memset and no allocation: every buffer lives in one caller-provided workspace, the frames go straight to
// the caller's [N,H,W,3] byte array — device memory, or pinned host memory the device can write.  The projection, binning and
// composite kernels are the ones a no-grad render() runs, called through the same frame functions (common.h, gs_frame_*) with
// the frame's pose as their only context: the projection clears the per-tile counters on its way, as in a stateless render.
#include <stdlib.h>
#include <string.h>
#include "common.h"

namespace {

constexpr int RGB8_VEC = 4;   // pixels per thread: one float4 per plane in, 12 interleaved bytes out

struct Rgb8x4 { uint32_t a, b, c; };   // four interleaved pixels: R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 (little endian)

// torchvision.utils.save_image's conversion (reference render.py:91-93), x.mul(255).add_(0.5).clamp_(0, 255).to(uint8): an fp32
// multiply rounded once, an fp32 add rounded once, the clamp, truncation.  A NaN gives 0 (torch leaves that conversion undefined).
__device__ __forceinline__ uint32_t rgb8_quantize(float x) {
#pragma clang fp contract(off)   // two roundings, as the two elementwise kernels of the expression: no fused multiply-add
  const float y = x * 255.0f;
  const float z = y + 0.5f;
  return z > 0.0f ? (uint32_t)fminf(z, 255.0f) : 0u;   // (a NaN fails the comparison)
}

// img [3,npix] planar -> out [npix,3] interleaved.  With npix a multiple of 4 and the pointers aligned (uniform over the launch)
// a thread loads one float4 per plane and stores its 12 bytes as one three-word record; otherwise — the planes of an image
// whose size is not a multiple of 4 do not all start on a 16-byte boundary — every thread walks its pixels, the tail included,
// in plain C++.  count_dst (may be null): the frame's instance count, copied by one lane so that it needs no launch of its own.
__global__ __launch_bounds__(256) void k_rgb8_from_planar(int npix, const float* __restrict__ img, uint8_t* __restrict__ out,
                                                          const uint32_t* __restrict__ count_src, int32_t* __restrict__ count_dst) {
  if (count_dst && blockIdx.x == 0 && threadIdx.x == 0) *count_dst = (int32_t)*count_src;
  const int i0 = (int)(blockIdx.x * 256u + threadIdx.x) * RGB8_VEC;
  if (i0 >= npix) return;
  const float* __restrict__ r = img;
  const float* __restrict__ g = img + npix;
  const float* __restrict__ b = img + 2 * (size_t)npix;
  if ((npix & (RGB8_VEC - 1)) == 0 && (((uintptr_t)img & 15) | ((uintptr_t)out & 3)) == 0) {
    const float4 R = reinterpret_cast<const float4*>(r)[i0 >> 2], G = reinterpret_cast<const float4*>(g)[i0 >> 2],
                 B = reinterpret_cast<const float4*>(b)[i0 >> 2];
    Rgb8x4 p;
    p.a = rgb8_quantize(R.x) | rgb8_quantize(G.x) << 8 | rgb8_quantize(B.x) << 16 | rgb8_quantize(R.y) << 24;
    p.b = rgb8_quantize(G.y) | rgb8_quantize(B.y) << 8 | rgb8_quantize(R.z) << 16 | rgb8_quantize(G.z) << 24;
    p.c = rgb8_quantize(B.z) | rgb8_quantize(R.w) << 8 | rgb8_quantize(G.w) << 16 | rgb8_quantize(B.w) << 24;
    *reinterpret_cast<Rgb8x4*>(out + 3 * (size_t)i0) = p;
  } else {
    const int i1 = min(npix, i0 + RGB8_VEC);
    for (int i = i0; i < i1; ++i) {
      out[3 * (size_t)i] = (uint8_t)rgb8_quantize(r[i]);
      out[3 * (size_t)i + 1] = (uint8_t)rgb8_quantize(g[i]);
      out[3 * (size_t)i + 2] = (uint8_t)rgb8_quantize(b[i]);
    }
  }
}

// every pixel index and i0 above fit an int
bool rgb8_size_ok(int W, int H) { return W > 0 && H > 0 && (long long)W * H <= 0x7fffffffLL - 256 * RGB8_VEC; }

int launch_rgb8(hipStream_t stream, int W, int H, const float* img, uint8_t* out, const uint32_t* count_src, int32_t* count_dst) {
  const int npix = W * H;
  const int per_block = 256 * RGB8_VEC;
  GS_KRANGE("rgb8_from_planar");
  hipLaunchKernelGGL(k_rgb8_from_planar, dim3((npix + per_block - 1) / per_block), dim3(256), 0, stream, npix, img, out, count_src,
                     count_dst);
  GS_CHECK_LAUNCH("rgb8_from_planar");
  return MI355GS_OK;
}

typedef GsFrozenScene Path;   // nothing of its own: render-only buffers, which no knob enters

size_t carve(Path& t, void* workspace) {
  GsCarver c{(char*)workspace};
  t.carve(c, gs_knobs(), false);
  return c.off;
}

}  // namespace

extern "C" {

int mi355gs_rgb8_from_planar(void* stream, int H, int W, const float* img, uint8_t* out) {
  GS_RANGE();
  if (!img || !out || !rgb8_size_ok(W, H)) return MI355GS_EINVAL;
  return launch_rgb8((hipStream_t)stream, W, H, img, out, nullptr, nullptr);
}

size_t mi355gs_path_workspace_bytes(int P, int W, int H, int64_t capacity) {
  if (P <= 0 || !rgb8_size_ok(W, H) || capacity <= 0) return 0;
  Path t;
  memset(&t, 0, sizeof(t));
  t.P = P; t.W = W; t.H = H; t.capacity = capacity;
  return carve(t, nullptr);
}

void* mi355gs_path_create(int P, int M, int W, int H, int64_t capacity, const float* xyz, const float* f_dc, const float* f_rest,
                          const float* opacity, const float* scaling, const float* rotation, void* workspace) {
  if (!rgb8_size_ok(W, H)) return nullptr;
  Path* t = (Path*)calloc(1, sizeof(Path));
  if (!t) return nullptr;
  if (!t->init(P, M, W, H, capacity, xyz, f_dc, f_rest, opacity, scaling, rotation, workspace)) { free(t); return nullptr; }
  carve(*t, workspace);
  return t;
}

void mi355gs_path_destroy(void* handle) { free(handle); }

int mi355gs_path_render(void* handle, void* stream_, int sh_degree, const float* projmatrix, float tanfovx, float tanfovy,
                        const float* bg, const float* poses, int first, int n, uint8_t* frames, int32_t* counts) {
  GS_RANGE();
  Path* t = (Path*)handle;
  hipStream_t stream = (hipStream_t)stream_;
  if (!t || !t->degree_ok(sh_degree) || !projmatrix || !bg || !poses || !frames || !counts) return MI355GS_EINVAL;
  if (first < 0 || n < 0 || n > 0x7fffffff - first) return MI355GS_EINVAL;
  if (n == 0) return MI355GS_OK;
  int rc;
  // The constants are written at the head of EVERY call, on that call's stream (a 2 us launch against n frames of ~120): a handle may
  // then be used on any stream, one call at a time, without an ordering between the call that first wrote them and a later one elsewhere.
  if ((rc = gs_write_view_consts(stream, t->consts, "view_consts"))) return rc;
  const GsScene scene = t->scene(sh_degree);
  const GsView view = t->view(projmatrix, tanfovx, tanfovy);
  const GsFrameBufs bufs = t->bufs(gs_knobs(), nullptr);
  const size_t frame_bytes = (size_t)t->W * t->H * 3;
  for (int i = first; i < first + n; ++i) {
    GsFrameCtx cx;
    cx.posed.pose = poses + 7 * (size_t)i;
    if ((rc = gs_frame_project(stream, scene, view, bufs, cx, t->num_rendered, nullptr, 0))) return rc;
    if ((rc = gs_frame_render(stream, t->P, view, bufs, bg, t->image, false, 0))) return rc;
    if ((rc = launch_rgb8(stream, t->W, t->H, t->image, frames + frame_bytes * (size_t)i, t->count(), counts + i))) return rc;
  }
  return MI355GS_OK;
}

}  // extern "C"
