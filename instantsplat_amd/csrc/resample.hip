// Resizing 8-bit RGB images behind one library call (include/mi355gs.h, mi355gs_resample_rgb8): PIL's `Image.resize` for 8-bit
// images (libImaging Resample.c, ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc), byte for byte.
//
//   horizontal pass: images [N,H,W,3] -> intermediate [N,rows,w,3], 8 bits (only the window's columns, only the source rows the
//                    window's vertical taps reach)
//   vertical pass:   intermediate -> the window [N,h,w,3] of the resized image, as bytes and / or as float planes
//
// Integer arithmetic throughout: per output value acc = 2^21 + sum_t k[t] * byte[min + t] in 32 bits, clip(acc >> 22, 0, 255).  The
// coefficient tables (22 fractional bits) and the tap bounds are the caller's (instantsplat_amd/resample.py builds them as PIL's
// precompute_coeffs does, in doubles on the host): no sin() on the device.  The intermediate is 8 bits wide, clipped, as PIL's is:
// a wider one gives other bytes where a negative lobe overshoots.  A pass whose size does not change is skipped (PIL skips it);
// the last pass that runs writes every selected output, so a call is two launches, or one.  The float outputs are the two
// conversions the reference applies to a resized image (utils/general_utils.py:21-27 PILtoTorch; ToTensor + Normalize(0.5, 0.5) in
// dust3r/utils/image.py), every operation rounded once: this file is compiled with -ffp-contract=off (Makefile).
//
// One thread per output pixel (three channels), lanes along x.  Rows of 3-byte pixels do not start on 4 bytes for arbitrary
// widths, and a tap window starts at any pixel, so every access is a byte access in plain C++ (path.hip's general path); the taps
// of neighbouring lanes overlap almost entirely, so the loads are served by the vector L1.  In the vertical pass a wave's lanes
// share the output row: the coefficient of a tap is one address for the whole wave.  In the horizontal pass every lane has its own
// table row, and a thread amortises each coefficient load over RS_ROWS source rows.
#include "common.h"

namespace {

constexpr int RS_BITS = 22;    // PIL's PRECISION_BITS for 8-bit images: 32 - 8 - 2
constexpr int RS_TX = 64;      // block: RS_TX columns x RS_TY rows of threads
constexpr int RS_TY = 4;
constexpr int RS_ROWS = 4;     // source rows per thread in the horizontal pass
constexpr int RS_MAX = 65535;  // every size and N (a grid dimension)

struct RsOut {                 // the window's outputs; a null pointer: not produced
  uint8_t* rgb8;               // [N,h,w,3]
  float* unit;                 // [N,3,h,w]  float(v) / 255
  float* normalized;           // [N,3,h,w]  (float(v) / 255 - 0.5) / 0.5
  int w, h;
};

// A coefficient as the multiplier takes it: its low 24 bits, signed.  PIL's stay below 2^23 in magnitude (a weight is at most a little
// above 1, 2^22), and a product of a 24-bit and an 8-bit factor is one full-rate v_mad_i32_i24 where a 32-bit one is a quarter-rate
// v_mad_u64_u32.  The sums wrap as unsigned ones: no table content is undefined behaviour.
__device__ __forceinline__ int32_t rs_coef(int32_t k) { return (int32_t)((uint32_t)k << 8) >> 8; }
__device__ __forceinline__ uint32_t rs_mad(int32_t c, uint8_t byte, uint32_t acc) { return acc + (uint32_t)(c * (int32_t)byte); }

__device__ __forceinline__ uint32_t rs_clip8(uint32_t acc) { return (uint32_t)min(max((int32_t)acc >> RS_BITS, 0), 255); }

// x, y: inside the window
__device__ __forceinline__ void rs_emit(const RsOut& o, int n, int y, int x, const uint32_t v[3]) {
  const size_t pix = (size_t)y * o.w + x, plane = (size_t)o.h * o.w;
  if (o.rgb8) {
    uint8_t* p = o.rgb8 + 3 * ((size_t)n * plane + pix);
    p[0] = (uint8_t)v[0]; p[1] = (uint8_t)v[1]; p[2] = (uint8_t)v[2];
  }
  for (int c = 0; c < 3; ++c) {
    const float u = (float)v[c] / 255.0f;   // IEEE division, as torch's
    const size_t i = ((size_t)n * 3 + c) * plane + pix;
    if (o.unit) o.unit[i] = u;
    if (o.normalized) o.normalized[i] = (u - 0.5f) / 0.5f;
  }
}

// Horizontal pass over the rows r0 .. r0+rows-1 of the source and the columns x0 .. x0+w-1 of the resized image.
// FINAL: the vertical pass is skipped (r0 = the window's first row, rows = its height): the outputs are written here.
// Otherwise tmp [N,rows,w,3] receives the bytes.  The tap range is clamped to the table row and to the source row, so that no
// table content reads outside the images.
template <bool FINAL>
__global__ __launch_bounds__(RS_TX * RS_TY) void k_resample_h(int H, int W, const uint8_t* __restrict__ src, const int32_t* __restrict__ kx,
                                                              const int32_t* __restrict__ bx, int ksize, int x0, int w, int r0, int rows,
                                                              uint8_t* __restrict__ tmp, RsOut out) {
  const int x = (int)(blockIdx.x * RS_TX + threadIdx.x);
  const int rb = (int)(blockIdx.y * RS_TY + threadIdx.y) * RS_ROWS;
  const int n = (int)blockIdx.z;
  if (x >= w || rb >= rows) return;
  const int xx = x0 + x;
  const int xmin = min(max(bx[2 * xx], -ksize), W);   // (beyond either end there is no tap left: the clamp only keeps the sums below in range)
  const int t0 = max(0, -xmin), t1 = min(min(bx[2 * xx + 1], ksize), W - xmin);
  const int32_t* __restrict__ k = kx + (size_t)xx * ksize;
  const uint8_t* p[RS_ROWS];
  uint32_t acc[RS_ROWS][3];
  for (int i = 0; i < RS_ROWS; ++i) {
    const int row = r0 + min(rb + i, rows - 1);   // a thread past the last row repeats it and stores nothing
    p[i] = src + 3 * (((size_t)n * H + row) * W + xmin);
    acc[i][0] = acc[i][1] = acc[i][2] = 1u << (RS_BITS - 1);
  }
  for (int t = t0; t < t1; ++t) {
    const int32_t c = rs_coef(k[t]);
    for (int i = 0; i < RS_ROWS; ++i) {
      acc[i][0] = rs_mad(c, p[i][3 * t], acc[i][0]);
      acc[i][1] = rs_mad(c, p[i][3 * t + 1], acc[i][1]);
      acc[i][2] = rs_mad(c, p[i][3 * t + 2], acc[i][2]);
    }
  }
  for (int i = 0; i < RS_ROWS && rb + i < rows; ++i) {
    const uint32_t v[3] = {rs_clip8(acc[i][0]), rs_clip8(acc[i][1]), rs_clip8(acc[i][2])};
    if (FINAL) {
      rs_emit(out, n, rb + i, x, v);
    } else {
      uint8_t* q = tmp + 3 * (((size_t)n * rows + rb + i) * w + x);
      q[0] = (uint8_t)v[0]; q[1] = (uint8_t)v[1]; q[2] = (uint8_t)v[2];
    }
  }
}

// Vertical pass to the window.  src: [N,rows,sw,3], holding the rows r0 .. r0+rows-1 of the image the tap bounds speak of; the
// window's column x is its column sx0 + x.  (The intermediate: sw = w, sx0 = 0.  The source itself when the horizontal pass is
// skipped: sw = W, sx0 = x0, r0 = 0, rows = H.)  Taps outside those rows are not read.
__global__ __launch_bounds__(RS_TX * RS_TY) void k_resample_v(const uint8_t* __restrict__ src, int sw, int sx0, int r0, int rows,
                                                              const int32_t* __restrict__ ky, const int32_t* __restrict__ by, int ksize,
                                                              int y0, RsOut out) {
  const int x = (int)(blockIdx.x * RS_TX + threadIdx.x);
  const int y = (int)(blockIdx.y * RS_TY + threadIdx.y);
  const int n = (int)blockIdx.z;
  if (x >= out.w || y >= out.h) return;
  const int yy = y0 + y;
  const int ymin = min(max(by[2 * yy], r0 - ksize), r0 + rows) - r0;   // (clamped as xmin is in the horizontal pass)
  const int t0 = max(0, -ymin), t1 = min(min(by[2 * yy + 1], ksize), rows - ymin);
  const int32_t* __restrict__ k = ky + (size_t)yy * ksize;
  const uint8_t* __restrict__ p = src + 3 * (((size_t)n * rows + ymin) * sw + sx0 + x);
  const size_t stride = 3 * (size_t)sw;
  uint32_t acc[3] = {1u << (RS_BITS - 1), 1u << (RS_BITS - 1), 1u << (RS_BITS - 1)};
  for (int t = t0; t < t1; ++t) {
    const int32_t c = rs_coef(k[t]);
    const uint8_t* q = p + (ptrdiff_t)t * (ptrdiff_t)stride;
    acc[0] = rs_mad(c, q[0], acc[0]);
    acc[1] = rs_mad(c, q[1], acc[1]);
    acc[2] = rs_mad(c, q[2], acc[2]);
  }
  const uint32_t v[3] = {rs_clip8(acc[0]), rs_clip8(acc[1]), rs_clip8(acc[2])};
  rs_emit(out, n, y, x, v);
}

// Neither size changes: the window of the source, converted (PIL copies the image).
__global__ __launch_bounds__(RS_TX * RS_TY) void k_resample_copy(int H, int W, const uint8_t* __restrict__ src, int x0, int y0, RsOut out) {
  const int x = (int)(blockIdx.x * RS_TX + threadIdx.x);
  const int y = (int)(blockIdx.y * RS_TY + threadIdx.y);
  const int n = (int)blockIdx.z;
  if (x >= out.w || y >= out.h) return;
  const uint8_t* p = src + 3 * (((size_t)n * H + y0 + y) * W + x0 + x);
  const uint32_t v[3] = {p[0], p[1], p[2]};
  rs_emit(out, n, y, x, v);
}

bool rs_dim_ok(int a) { return a > 0 && a <= RS_MAX; }
// the bytes of one image fit an int (the kernels' offsets are size_t; the limit keeps every grid dimension in range as well)
bool rs_image_ok(int H, int W) { return rs_dim_ok(H) && rs_dim_ok(W) && 3ll * H * W <= 0x7fffffffll; }

}  // namespace

extern "C" {

size_t mi355gs_resample_rgb8_scratch_bytes(int N, int rows, int w) {
  if (!rs_dim_ok(N) || !rs_image_ok(rows, w)) return 0;
  return ((size_t)N * rows * w * 3 + 15) & ~(size_t)15;
}

int mi355gs_resample_rgb8(void* stream_, int N, int H, int W, int Hout, int Wout, const uint8_t* images, const int32_t* kx,
                          const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, int x0, int y0, int w, int h,
                          int row0, int rows, void* scratch, uint8_t* rgb8, float* unit, float* normalized) {
  GS_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (!rs_dim_ok(N) || !rs_image_ok(H, W) || !rs_image_ok(Hout, Wout) || !images || (!rgb8 && !unit && !normalized)) return MI355GS_EINVAL;
  if (x0 < 0 || y0 < 0 || w <= 0 || h <= 0 || w > Wout - x0 || h > Hout - y0) return MI355GS_EINVAL;
  const bool horizontal = kx != nullptr, vertical = ky != nullptr;
  if (horizontal ? (!bx || ksize_x <= 0) : Wout != W) return MI355GS_EINVAL;
  if (vertical ? (!by || ksize_y <= 0) : Hout != H) return MI355GS_EINVAL;
  if (horizontal && vertical && (!scratch || row0 < 0 || rows <= 0 || rows > H - row0)) return MI355GS_EINVAL;
  const RsOut out{rgb8, unit, normalized, w, h};
  const dim3 block(RS_TX, RS_TY);
  const dim3 grid((w + RS_TX - 1) / RS_TX, (h + RS_TY - 1) / RS_TY, N);
  if (horizontal) {
    const int r0 = vertical ? row0 : y0, nr = vertical ? rows : h;
    const dim3 hgrid((w + RS_TX - 1) / RS_TX, (nr + RS_TY * RS_ROWS - 1) / (RS_TY * RS_ROWS), N);
    GS_KRANGE("resample_h");
    if (vertical)
      hipLaunchKernelGGL(k_resample_h<false>, hgrid, block, 0, stream, H, W, images, kx, bx, ksize_x, x0, w, r0, nr, (uint8_t*)scratch, out);
    else
      hipLaunchKernelGGL(k_resample_h<true>, hgrid, block, 0, stream, H, W, images, kx, bx, ksize_x, x0, w, r0, nr, (uint8_t*)nullptr, out);
    GS_CHECK_LAUNCH("resample_h");
  }
  if (vertical) {
    GS_KRANGE("resample_v");
    if (horizontal)
      hipLaunchKernelGGL(k_resample_v, grid, block, 0, stream, (const uint8_t*)scratch, w, 0, row0, rows, ky, by, ksize_y, y0, out);
    else
      hipLaunchKernelGGL(k_resample_v, grid, block, 0, stream, images, W, x0, 0, H, ky, by, ksize_y, y0, out);
    GS_CHECK_LAUNCH("resample_v");
  }
  if (!horizontal && !vertical) {
    GS_KRANGE("resample_copy");
    hipLaunchKernelGGL(k_resample_copy, grid, block, 0, stream, H, W, images, x0, y0, out);
    GS_CHECK_LAUNCH("resample_copy");
  }
  return MI355GS_OK;
}

}  // extern "C"
