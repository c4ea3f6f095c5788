// Shared definitions for the gfx950 kernels of libmi355gs.so.
// Scratch-buffer layouts (all offsets 256-byte aligned) are defined here once so that the
// size queries, the forward and the backward agree.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/mi355gs.h"
#include <type_traits>

#define GS_LOG2E 1.4426950408889634f
#define GS_TILE 16
#define GS_TILE_PIX 256
#define GS_WAVE 64

// One 48-byte record per Gaussian, written by preprocess and gathered by the composite kernels
// with three 16-byte loads from one contiguous address (1 cache line most of the time).
struct alignas(16) GsRec {
  float4 q0;  // x, y (pixel centre), hx, hy (half extents of the alpha >= 1/255 ellipse's AABB; <0: never visible)
  float4 q1;  // conic pre-scaled for v_exp_f32 and ordered for packed-FP32 math: (-a/2, -c/2, -b) * log2(e), then
              // opacity — so that G = exp2(q1.x*dx*dx + q1.y*dy*dy + q1.z*dx*dy) with no further multiplies and
              // (q1.x, q1.y) * (dx, dy) is one v_pk_mul_f32
  float4 q2;  // r, g, b, depth
};

// Per-Gaussian accumulator filled by composite backward (float atomics): moments of w = G * dL/dG over all
// pixels the Gaussian touched, plus the colour gradient.  k_preprocess_bwd turns the moments into
// dL/dmean2D, dL/dconic and dL/dopacity with the Gaussian's own conic and opacity.
struct alignas(16) GsGrad {
  float4 g0;  // sum w dx, sum w dy, sum w dx^2, sum w dx dy
  float4 g1;  // sum w dy^2, sum w, dL/dr, dL/dg
  float4 g2;  // dL/db, unused x3
};

static inline size_t gs_align(size_t x) { return (x + 255) & ~(size_t)255; }

// Carves a handle's buffers out of one caller-provided workspace (trainer, tracker, path): take<T>(n) returns the next
// 256-byte-aligned block of n elements; with a null base it only counts, which is how the *_workspace_bytes queries size it.
struct GsCarver {
  char* base;
  size_t off = 0;
  template <class T> T* take(size_t n) {
    T* p = base ? (T*)(base + off) : nullptr;
    off += gs_align(n * sizeof(T));
    return p;
  }
};
// The device constants InstantSplat's render() hands the operator (reference gaussian_renderer/__init__.py:55-59), written by
// one tiny launch (api.hip): consts[0..15] = the identity view matrix, consts[16..18] = the camera position 0.  `name`: the
// launch's range in a marker trace.
int gs_write_view_consts(hipStream_t stream, float* consts, const char* name);

// Binning (binning.hip): a workgroup counts / scatters GS_BIN_CHUNK consecutive Gaussians; the count kernel leaves each
// workgroup's touched tiles as up to GS_BIN_ENTRIES packed (tile | count << 16) words for the scatter kernel of the same frame.
constexpr int GS_BIN_CHUNK = 512;
constexpr int GS_BIN_ENTRIES = 1024;

struct GeomLayout {
  size_t rec, cov3D, rect, clamped, depth, bin_entries, bin_n, total;
  __host__ explicit GeomLayout(int P) {
    size_t n = P > 0 ? (size_t)P : 1, o = 0;
    rec = o; o += gs_align(n * sizeof(GsRec));
    cov3D = o; o += gs_align(n * 6 * sizeof(float));
    rect = o; o += gs_align(n * sizeof(uint2));
    clamped = o; o += gs_align(n);
    depth = o; o += gs_align(n * sizeof(float));   // the view depth once more, densely: the scatter reads 4 B per Gaussian, not a 48-B record's line
    const size_t chunks = (n + GS_BIN_CHUNK - 1) / GS_BIN_CHUNK;
    bin_entries = o; o += gs_align(chunks * GS_BIN_ENTRIES * sizeof(uint32_t));
    bin_n = o; o += gs_align(chunks * sizeof(uint32_t));
    total = o;
  }
};

constexpr int GS_SORT_SMALL_CAP = 2048;  // keys the tile sort's register network takes in one go (binning.hip)

constexpr int GS_UNIT_LEVELS = 4;
// The rule, shared by the device (k_scan_tiles, from the frame's true instance count) and the host (from the capacity, to
// pick the kernel instantiation and to size buffers): lengthen the units while at least `min_units` of them remain.
__host__ __device__ inline int gs_unit_level_for(long long instances, long long min_units) {
  int level = 0;
  while (level + 1 < GS_UNIT_LEVELS && (instances >> (7 + level)) >= min_units) ++level;   // instances / (2 * 64 << level), instances >= 0
  return level;
}
// Deterministic-backward mode (mi355gs_tune_deterministic, composite.hip): the moments of every (Gaussian, tile) instance go to a
// row of their own and are summed per Gaussian in tile order instead of meeting in float atomics.  It enters the layouts below
// (rows + row indices per instance in `binning`, the per-Gaussian row offsets behind the gate flags in the gradient scratch).
// The two knobs that enter buffer layouts.  A layout is a function of the values it is handed: the public size queries and the
// stateless operators pass gs_knobs(), a handle passes the values it snapshotted when its workspace was carved.
struct GsKnobs {
  int min_units;  // mi355gs_tune_min_units (binning.hip): lengthen the backward's units only while at least this many remain
  int det;        // mi355gs_tune_deterministic (api.hip)
};
GsKnobs gs_knobs();               // api.hip: the process-wide knobs as they stand now
struct DetScratchLayout {         // behind the 256 bytes of gate flags in the gradient scratch; all uint32
  size_t off, block_sums, total;
  __host__ explicit DetScratchLayout(int P) {
    const size_t n = (size_t)(P > 0 ? P : 1) + 1;
    size_t o = 0;
    off = o; o += gs_align((n + 1) * 4);             // exclusive prefix sums of the rectangles' tile counts: first row of Gaussian g
    block_sums = o; o += gs_align(((n + 4095) / 4096 + 2) * 4);
    total = o;
  }
};
int gs_min_units();               // binning.hip: the mi355gs_tune_min_units knob
constexpr int GS_MIN_UNITS = 40960;  // lengthen units only while at least this many remain (6-7 rounds of the 6144 resident waves:
                                     // measured at C4, 7.3 M instances: 512-instance units 2.34 ms/view, 256: 2.28, 128: 2.21, 64: 2.24)

struct TilesLayout {
  size_t count, start, cursor, final_T, n_contrib, order, seg_first, part_first, meta, qmax, total;
  int gx, gy, T;
  __host__ TilesLayout(int W, int H) {
    gx = (W + GS_TILE - 1) / GS_TILE; gy = (H + GS_TILE - 1) / GS_TILE; T = gx * gy;
    size_t o = 0, npix = (size_t)W * H;
    count = o; o += gs_align((size_t)T * 4);
    cursor = o; o += gs_align((size_t)T * 4);   // count and cursor are adjacent: one memset clears both
    start = o; o += gs_align(((size_t)T + 1) * 4);
    final_T = o; o += gs_align(npix * 4);
    n_contrib = o; o += gs_align(npix * 4);
    order = o; o += gs_align((size_t)T * 4);
    seg_first = o; o += gs_align(((size_t)T + 1) * 4);  // prefix over tiles of ceil(count / unit length): first unit of a tile
    part_first = o; o += gs_align(((size_t)T + 1) * 4);  // prefix over tiles of "the tile's last unit is shorter than the unit length"
    meta = o; o += gs_align(16);   // [1]: backward units of the frame, [2]: chunks of GS_SEG instances per unit, [3]: short units
    qmax = o; o += gs_align((size_t)T * 4 * 4);   // per tile and 8x8 quadrant: the largest per-pixel contributor count (forward -> backward)
    total = o;
  }
};

// Backward work units: a tile's depth-ordered list is cut into segments of GS_SEG instances.  The forward composite
// leaves each pixel's (transmittance, accumulated colour) at every segment boundary, so the backward can replay the
// segments independently: thousands of equal-sized workgroups that the hardware balances, instead of one workgroup per
// tile that lasts as long as the tile is deep (composite.hip).
constexpr int GS_SEG = 64;
// A unit covers 1, 2, 4 or 8 consecutive 64-instance chunks ("level" 0..3), chosen per frame by k_scan_tiles from the frame's
// true instance count and left in meta[2]: boundaries — and with them the 16 B/pixel boundary records and the 32 B/pixel of
// per-pixel state a unit loads — are only needed every (64 << level) instances.  At C3 (0.75 M instances) that is one chunk; at
// C4 (7.3 M) eight: the boundary state touched per frame falls from 700 MB to under 90 MB.  The host only needs to know whether
// the looping instantiation of the backward can be required (level of the CAPACITY > 0; count <= capacity) and an upper bound
// on the number of units for the buffers.

struct BinningLayout {
  size_t keys, list, unit_tile, bstate, hitmask, det_rows, det_rowidx, total;
  uint32_t max_chunks;  // 64-instance chunks the hit-mask table has room for
  uint32_t max_units;  // table / boundary slots available: an upper bound on the units of any frame with <= R instances
  bool may_loop;       // a frame with this capacity can have units longer than one chunk
  __host__ BinningLayout(int64_t R, int T, const GsKnobs& knobs) {
    size_t n = R > 0 ? (size_t)R : 1, o = 0;
    keys = o; o += gs_align(n * 8);
    list = o; o += gs_align(n * 4);
    // A frame with c <= R instances runs at level L(c) <= L(R) and has at most c / (64 << L(c)) + T units (one partial unit per
    // tile).  While L(c) is below the top level the rule stopped lengthening, so c / (64 << L(c)) < 2 * min_units; at the top
    // level it is at most R / (64 << top).  Small capacities never exceed ceil(R / 64).
    const size_t mu = (size_t)knobs.min_units, top = (size_t)GS_SEG << (GS_UNIT_LEVELS - 1);
    const size_t by_chunks = (n + GS_SEG - 1) / GS_SEG, by_rule = 2 * mu + 1, by_top = (n + top - 1) / top;
    const size_t lim = by_chunks < by_rule ? by_chunks : by_rule;
    may_loop = gs_unit_level_for((long long)n, (long long)mu) > 0;
    max_units = (uint32_t)((lim > by_top ? lim : by_top) + (size_t)(T > 0 ? T : 1));
    unit_tile = o; o += gs_align((size_t)max_units * 16);  // uint4 per unit, in launch order: (tile x | tile y << 16, segment, slot, 0)
    bstate = o; o += gs_align((size_t)max_units * 256 * sizeof(float4));  // per boundary: 256 pixels x (T, C0, C1, C2)
    // Per 64-instance chunk of a tile's list, the four quadrants' hit masks the forward's cull produced (which of the chunk's
    // instances can reach alpha >= 1/255 somewhere in the quadrant): the backward reads them instead of repeating the test
    // (4 x ~60 VALU instructions per unit).  Chunk index = (first unit of the tile + unit) * chunks per unit + chunk, which is
    // below instances / 64 + 8 per tile at every unit length.
    max_chunks = (uint32_t)(by_chunks + 8 * (size_t)(T > 0 ? T : 1) + 8);
    hitmask = o; o += gs_align((size_t)max_chunks * 4 * sizeof(uint64_t));
    det_rows = det_rowidx = o;
    if (knobs.det) {   // one row of twelve floats (a GsGrad) and one row index per instance
      det_rows = o; o += gs_align(n * sizeof(GsGrad));
      det_rowidx = o; o += gs_align(n * 4);
    }
    total = o;
  }
};


// transposed (column-major flat) 4x4 helpers, the storage the reference hands over
__device__ __forceinline__ float3 gs_tp43(const float* m, float3 p) {
  return make_float3(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                     m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14]);
}
__device__ __forceinline__ float4 gs_tp44(const float* m, float3 p) {
  return make_float4(m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12], m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13],
                     m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14], m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15]);
}

struct CamParams {  // passed by value (kernarg): wave-uniform, lives in SGPRs
  const float* view;    // device pointers: uniform address -> scalar loads
  const float* proj;
  const float* campos;
  float tanfovx, tanfovy, focal_x, focal_y, scale_modifier;
  float scale_grad_factor;   // backward only: dL/dscale = factor x dL/d(scale_modifier * scale) — 1 (the published operator's
                             // convention, default) or scale_modifier (the true derivative), mi355gs_tune_scale_grad
  int W, H, gx, gy;
};

// DPP (data-parallel primitive) lane exchange of a 32- or 64-bit value (two moves): VALU ops, no LDS traffic.  Lanes without a
// source read zero bits.
template <int CTRL, int ROW_MASK = 0xF, class T>
__device__ __forceinline__ T gs_dpp(T v) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two 32-bit moves");
  uint32_t w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
  for (size_t i = 0; i < sizeof(T) / 4; ++i) w[i] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[i], CTRL, ROW_MASK, 0xF, false);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}
// wave64 sum in 6 DPP adds (a shuffle butterfly is six LDS-crossbar round trips, twelve for 64 bits); the total lands in lanes
// 48..63 (the last row of 16).  All lanes must be active.
template <class T>
__device__ __forceinline__ T gs_wave_sum_row3(T v) {
  v += gs_dpp<0xB1>(v);        // quad_perm [1,0,3,2]
  v += gs_dpp<0x4E>(v);        // quad_perm [2,3,0,1]
  v += gs_dpp<0x141>(v);       // row_half_mirror
  v += gs_dpp<0x140>(v);       // row_mirror        -> every lane holds its row's sum
  v += gs_dpp<0x142, 0xA>(v);  // row_bcast:15 into rows 1,3
  v += gs_dpp<0x143, 0xC>(v);  // row_bcast:31 into rows 2,3 -> row 3 holds the wave total
  return v;
}
__device__ __forceinline__ double gs_wave_sum_row3_f64(double v) { return gs_wave_sum_row3(v); }

// Two means from [nblocks, 2] float partial sums, for a workgroup of 1024 threads: double accumulation in a fixed order (strided
// per thread, DPP wave sum, the 16 wave totals in sequence), so every kernel that finishes the same partials leaves the same
// bits.  The results are valid in thread 0 only.
__device__ __forceinline__ void gs_finish_two_means(int nblocks, double inv_n, const float* __restrict__ partial, float& mean0, float& mean1) {
  __shared__ double s_a[16], s_b[16];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += 1024) { a += (double)partial[2 * i]; b += (double)partial[2 * i + 1]; }
  a = gs_wave_sum_row3(a); b = gs_wave_sum_row3(b);
  if ((threadIdx.x & 63) == 63) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double ta = 0.0, tb = 0.0;
  for (int w = 0; w < 16; ++w) { ta += s_a[w]; tb += s_b[w]; }
  mean0 = (float)(ta * inv_n); mean1 = (float)(tb * inv_n);
}
// the training loss from the two means (reference train.py:176)
__device__ __forceinline__ float gs_l1_ssim_loss(float lambda_dssim, float l1_mean, float ssim_mean) {
  return (1.0f - lambda_dssim) * l1_mean + lambda_dssim * (1.0f - ssim_mean);
}

// Two floats in an aligned VGPR pair: element-wise arithmetic on it compiles to CDNA3/4's full-rate packed-FP32 ops
// (v_pk_add/mul/fma_f32: two lanes' worth of work per issue slot).
typedef float gs_v2f __attribute__((vector_size(8)));
__device__ __forceinline__ gs_v2f gs_fma2(gs_v2f a, gs_v2f b, gs_v2f c) { return a * b + c; }  // contracted: v_pk_fma_f32

// wave64 maximum, in every lane: four DPP steps inside the rows, then the two row swaps (no LDS crossbar)
__device__ __forceinline__ uint32_t gs_wave_max_u32(uint32_t v) {
  auto dpp = [](uint32_t x, auto ctrl) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, decltype(ctrl)::value, 0xF, 0xF, true); };
  v = max(v, dpp(v, std::integral_constant<int, 0xB1>{}));   // quad_perm [1,0,3,2]
  v = max(v, dpp(v, std::integral_constant<int, 0x4E>{}));   // quad_perm [2,3,0,1]
  v = max(v, dpp(v, std::integral_constant<int, 0x141>{}));  // row_half_mirror
  v = max(v, dpp(v, std::integral_constant<int, 0x140>{}));  // row_mirror
  const auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);
  v = max(a[0], a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(v, v, false, false);
  return max(b[0], b[1]);
}

// wave64 inclusive prefix sum in six DPP adds (row_shr:1/2/4/8 inside the rows of 16, then row_bcast:15 and row_bcast:31 carry
// the row totals on): no LDS crossbar round trip per step (a __shfl_up is a ds_bpermute).  All lanes must be active.
__device__ __forceinline__ uint32_t gs_wave_scan_incl_u32(uint32_t v) {
  auto up = [](uint32_t x, auto ctrl, auto rows) {   // lanes without a source (or in a masked row) receive 0
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, decltype(ctrl)::value, decltype(rows)::value, 0xF, false);
  };
  using all = std::integral_constant<int, 0xF>;
  v += up(v, std::integral_constant<int, 0x111>{}, all{});   // row_shr:1
  v += up(v, std::integral_constant<int, 0x112>{}, all{});   // row_shr:2
  v += up(v, std::integral_constant<int, 0x114>{}, all{});   // row_shr:4
  v += up(v, std::integral_constant<int, 0x118>{}, all{});   // row_shr:8  -> inclusive scan inside every row
  v += up(v, std::integral_constant<int, 0x142>{}, std::integral_constant<int, 0xA>{});   // row_bcast:15 into rows 1 and 3
  v += up(v, std::integral_constant<int, 0x143>{}, std::integral_constant<int, 0xC>{});   // row_bcast:31 into rows 2 and 3
  return v;
}

// Sum over the four 16-lane rows, lane-wise (every lane ends with the sum of the lanes l, l^16, l^32, l^48), with
// gfx950's VALU row swaps — no LDS round trip (ds_bpermute) on the critical path.
__device__ __forceinline__ float gs_sum_rows(float v) {
  const unsigned u = __float_as_uint(v);
  const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  const float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const unsigned w = __float_as_uint(s);
  const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// physical CU of the calling wave (measurement builds: tools/probe_composite.py)
__device__ __forceinline__ uint32_t gs_physical_cu() {
  const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));   // HW_REG_HW_ID: cu_id [11:8], sh_id [12], se_id [14:13]
  const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11));  // HW_REG_XCC_ID [3:0]
  return ((xcc & 7u) << 6) | (((hw >> 13) & 3u) << 4) | ((hw >> 8) & 15u);
}

// ---- The f32-input matrix instruction (mm_tile.h: lpips.hip, vit.hip, dpt.hip): the accumulator type, 16 bytes moved at once,
// and the one helper that names the instruction.
#ifdef __clang__
typedef float lp_acc16 __attribute__((ext_vector_type(16)));
#else
struct lp_acc16 {
  float v[16];
  float& operator[](int i) { return v[i]; }
  float operator[](int i) const { return v[i]; }
};
#endif
// 16 bytes moved at once.  (Arrays of HIP's float4 class held across the K loop are not promoted to registers by hipcc.)
// LP_AT / LP_ATC: element k of one (hipcc: the vector type's own subscript, which stays in registers; g++: the struct's storage).
#ifdef __clang__
typedef float lp_f4 __attribute__((ext_vector_type(4)));
#define LP_AT(v, k) ((v)[k])
#define LP_ATC(v, k) ((v)[k])
#else
typedef float4 lp_f4;
#define LP_AT(v, k) (((float*)&(v))[k])
#define LP_ATC(v, k) (((const float*)&(v))[k])
#endif

// The one place the matrix instruction is named.  C (32x32, float32) += A (32x2) B (2x32) on one wave, the operands read from
// LDS: A[m][k] = As[m * lda + k], B[k][n] = Bs[k * ldb + n].  Lane l supplies A[l & 31][l >> 5] and B[l >> 5][l & 31] and holds
// C[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31] in register r.  The instruction rounds like the chain below (one rounding per
// product-and-add, k ascending), so the portable body — the host pass and the g++ build of the CPU test tier, where every lane
// reads its operands from the same LDS image — computes the same bits.
__device__ __forceinline__ void lp_mfma_32x32x2(lp_acc16& c, const float* As, int lda, const float* Bs, int ldb, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(lane & 31) * lda + (lane >> 5)], Bs[(lane >> 5) * ldb + (lane & 31)], c, 0, 0, 0);
#else
  for (int k = 0; k < 2; ++k) {
    const float b = Bs[k * ldb + (lane & 31)];
    for (int r = 0; r < 16; ++r) c[r] = fmaf(As[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * lda + k], b, c[r]);
  }
#endif
}

__device__ __forceinline__ int lp_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

extern thread_local bool g_krange_open;
void gs_range_pop();
void gs_log_error(const char* where, const char* what);
// Behind every launch: closes the launch's range (GS_KRANGE) and reports a launch error.  GS_CHECK_LAUNCH_SYNC is the form of
// the operators that have a `debug` argument (mi355gs_raster_*, mi355gs_posed_*): with debug != 0 it waits for the kernel too.
inline bool gs_launch_failed(const char* name, hipStream_t stream = nullptr, int debug = 0) {
  if (g_krange_open) { g_krange_open = false; gs_range_pop(); }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && debug) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) gs_log_error(name, hipGetErrorString(e));
  return e != hipSuccess;
}
#define GS_CHECK_LAUNCH(name) do { if (gs_launch_failed(name)) return MI355GS_ELAUNCH; } while (0)
#define GS_CHECK_LAUNCH_SYNC(name, stream, debug) do { if (gs_launch_failed(name, stream, debug)) return MI355GS_ELAUNCH; } while (0)

// roctx range around an entry point's launches (mi355gs_profile_ranges, api.hip): one predictable branch when off
extern bool g_ranges_on;
void gs_range_push(const char* name);
void gs_range_pop();
struct GsRange {
  bool active;
  explicit GsRange(const char* name) : active(g_ranges_on) { if (active) gs_range_push(name); }
  ~GsRange() { if (active) gs_range_pop(); }
  GsRange(const GsRange&) = delete;
  GsRange& operator=(const GsRange&) = delete;
};
#define GS_RANGE() GsRange gs_range_(__func__)
// ... and around ONE launch: GS_KRANGE("name") in front of it, popped by the GS_CHECK_LAUNCH("name") behind it
extern thread_local bool g_krange_open;
#define GS_KRANGE(name) do { if (g_ranges_on) { gs_range_push(name); g_krange_open = true; } } while (0)

// Optional in-library kernel timing (mi355gs_profile_*, api.hip): an event pair around the launches made in its scope, on the
// launch stream, when profiling is on and it is this launch's turn.  kind: include/mi355gs.h mi355gs_profile_read.
struct GsProfScope {
  hipStream_t s; hipEvent_t stop; bool active = false;
  GsProfScope(int kind, hipStream_t stream);
  ~GsProfScope();
};

// ---- One frame through the shared kernels (api.hip): what a call means is in its arguments.  The public mi355gs_raster_*
// entry points build these structs with a default GsFrameCtx; mi355gs_posed_*, the one-call train step (trainer.hip), the pose
// tracker (tracker.hip) and the camera-path renderer (path.hip) call the gs_frame_* functions with their own.

struct GsPrologue {  // accumulators of one frame, zeroed by the frame's first kernel (the projection) instead of memsets
  float4* grad_records = nullptr; size_t n_vec = 0;      // the 48-byte GsGrad records, as float4
  uint32_t* tile_counters = nullptr; int n_counters = 0;  // per-tile count + cursor
  float* g_poses = nullptr; int n_pose = 0;
  float* pose_scratch = nullptr;                           // 32 floats
  float* adam_scratch = nullptr;                           // 8 gate flags
};
// Posed projection: the projection kernels take the RAW parameters (xyz, raw quaternion, log-scale, opacity logit) plus
// the camera pose and apply InstantSplat's camera-frame transform / activations themselves (pose_math.h), and their
// backward goes all the way to the raw-parameter gradients and the 16 pose sums — no k_pose_fwd / k_pose_bwd launches
// and no camera-frame intermediates in HBM.
struct GsPosed {
  const float* pose = nullptr;  // [7] (qw,qx,qy,qz,tx,ty,tz); null = inputs are already in the camera frame
  float* acc = nullptr;         // backward: 16 pose sums (see pose_math.h), zeroed by the caller ...
  float* partial = nullptr;     // ... or, if set, one row of 16 per workgroup of the backward projection kernel (no atomics)
};
// "gradient tensor k has a non-zero" flags for PerPointAdam, written by the kernels that write the gradients (gate[k] > 0 <=>
// tensor k has a non-zero gradient) instead of a separate pass over all gradients: k in the optimizer's group order
enum { GS_GATE_XYZ = 0, GS_GATE_SH = 1, GS_GATE_SH_REST = 2, GS_GATE_OPACITY = 3, GS_GATE_SCALING = 4, GS_GATE_ROT = 5, GS_GATE_POSE = 6 };

struct GsScene {  // the Gaussians as the operator receives them
  int P, D, M;
  const float *means3D, *shs, *shs_rest, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
  float scale_modifier;
};
struct GsView {
  int W, H;
  const float *view, *proj, *campos;
  float tanfovx, tanfovy;
};
struct GsFrameBufs {  // the frame's scratch buffers (size queries of include/mi355gs.h) and the knobs they were laid out for
  void *geom, *tiles, *binning;
  int64_t capacity;   // instances `binning` holds
  int32_t* radii;
  void* grad_scratch;
  GsKnobs knobs;
};
struct GsFrameCtx {  // what a fused caller means beyond the operator's arguments; the default is the stateless operator
  const GsPrologue* prologue = nullptr;  // set: the projection clears exactly this list and the frame issues no memset of its own
  GsPosed posed;
  float* gate = nullptr;   // posed backward only: device float[8] of gate flags (GS_GATE_*), or null
  bool gate_tail = false;  // the flags live right behind the GsGrad records (mi355gs_raster_grad_gate_offset) and are cleared with them
  bool pose_only = false;  // pose tracking: with `posed` set the projection backward stops at the 16 pose sums — no per-Gaussian
                           // gradient, screen-space gradient or gate flag is stored, and every GsGradOut pointer may be null
};
struct GsGradOut { float *means3D, *means2D, *shs, *shs_rest, *colors, *opacities, *scales, *rotations, *cov3D; };
static inline size_t gs_grad_gate_offset(int P) { return gs_align((size_t)(P > 0 ? P : 1) * sizeof(GsGrad)); }
static inline size_t gs_grad_scratch_bytes(int P, int det) { return gs_grad_gate_offset(P) + 256 + (det ? DetScratchLayout(P).total : 0); }
static inline size_t gs_binning_bytes(int64_t n, int W, int H, const GsKnobs& k, bool train) {
  const BinningLayout bl(n, TilesLayout(W, H).T, k);
  return train ? bl.total : bl.unit_tile;   // render-only: keys + list, everything in front of the backward's tables
}
// W x H is a frame the kernels can take: the tile grid's dimensions are launch-grid dimensions
static inline bool gs_frame_size_ok(int W, int H) { return W > 0 && H > 0 && W <= 65535 * GS_TILE && H <= 65535 * GS_TILE; }
static inline uint32_t clamp_capacity(int64_t c) { return c <= 0 ? 0u : (c > 0x7fffffffLL ? 0x7fffffffu : (uint32_t)c); }

// Typed pointers into one frame's scratch buffers.  The layouts above say what a buffer contains; this is the one place that
// gives each field its type.  Built once per call from the buffers and (P, W, H > 0); a null buffer gives null pointers.
struct GsFrame {
  int P, W, H, T, gx;
  uint32_t cap;                        // instances `binning` holds, as the kernels take it
  // geom
  GsRec* recs; float* cov3D; uint2* rects; uint8_t* clamped; float* depths; uint32_t *bin_entries, *bin_n;
  // tiles
  uint32_t *count, *cursor, *start; float* final_T; uint32_t *n_contrib, *order, *seg_first, *part_first, *meta, *qmax;
  int n_counters;                      // count + cursor words: what a prologue clears
  // binning; the deterministic mode's rows are null outside it
  uint64_t* keys; uint32_t* list; uint4* unit_tile; float4* bstate; unsigned long long* hitmask; float* det_rows; uint32_t* det_rowidx;
  uint32_t max_units, max_chunks; bool may_loop;
  int32_t* radii; void* grad_scratch; GsKnobs knobs;

  GsFrame(const GsFrameBufs& fb, int P_, int W_, int H_)
      : P(P_), W(W_), H(H_), cap(clamp_capacity(fb.capacity)), radii(fb.radii), grad_scratch(fb.grad_scratch), knobs(fb.knobs) {
    const GeomLayout gl(P);
    const TilesLayout tl(W, H);
    const BinningLayout bl(fb.capacity, tl.T, fb.knobs);
    T = tl.T; gx = tl.gx;
    recs = at<GsRec>(fb.geom, gl.rec); cov3D = at<float>(fb.geom, gl.cov3D); rects = at<uint2>(fb.geom, gl.rect);
    clamped = at<uint8_t>(fb.geom, gl.clamped); depths = at<float>(fb.geom, gl.depth);
    bin_entries = at<uint32_t>(fb.geom, gl.bin_entries); bin_n = at<uint32_t>(fb.geom, gl.bin_n);
    count = at<uint32_t>(fb.tiles, tl.count); cursor = at<uint32_t>(fb.tiles, tl.cursor); start = at<uint32_t>(fb.tiles, tl.start);
    final_T = at<float>(fb.tiles, tl.final_T); n_contrib = at<uint32_t>(fb.tiles, tl.n_contrib); order = at<uint32_t>(fb.tiles, tl.order);
    seg_first = at<uint32_t>(fb.tiles, tl.seg_first); part_first = at<uint32_t>(fb.tiles, tl.part_first);
    meta = at<uint32_t>(fb.tiles, tl.meta); qmax = at<uint32_t>(fb.tiles, tl.qmax);
    n_counters = (int)((tl.start - tl.count) / 4);
    keys = at<uint64_t>(fb.binning, bl.keys); list = at<uint32_t>(fb.binning, bl.list);   // (the render-only buffer ends here)
    unit_tile = at<uint4>(fb.binning, bl.unit_tile); bstate = at<float4>(fb.binning, bl.bstate);
    hitmask = at<unsigned long long>(fb.binning, bl.hitmask);
    det_rows = at<float>(knobs.det ? fb.binning : nullptr, bl.det_rows);
    det_rowidx = at<uint32_t>(knobs.det ? fb.binning : nullptr, bl.det_rowidx);
    max_units = bl.max_units; max_chunks = bl.max_chunks; may_loop = bl.may_loop;
  }
  // a view of `tiles` alone (frame statistics, the frame's count): only the tiles fields, T and gx mean anything in it
  GsFrame(void* tiles, int W_, int H_) : GsFrame({nullptr, tiles, nullptr, 0, nullptr, nullptr, GsKnobs{GS_MIN_UNITS, 0}}, 0, W_, H_) {}

 private:
  template <class T_> static T_* at(void* base, size_t off) { return base ? (T_*)((char*)base + off) : nullptr; }
};
// the frame's true instance count: tile_start[T], written by the tile scan
static inline const uint32_t* gs_frame_count(const void* tiles, int W, int H) {
  const GsFrame f(const_cast<void*>(tiles), W, H);
  return f.start + f.T;
}

// ---- The launchers, each implemented next to its kernels.  A launcher over a frame takes the view and what is not in it.
// preprocess.hip: projection forward / backward (`grads`: the composite backward's moment records), reference markVisible
int gs_launch_preprocess_fwd(hipStream_t stream, const GsScene& sc, const CamParams& cp, const GsFrame& f, uint8_t* visible,
                             const GsPosed& posed_args, const GsPrologue& pro);
int gs_launch_preprocess_bwd(hipStream_t stream, const GsScene& sc, const CamParams& cp, const GsFrame& f, const GsGrad* grads,
                             const GsGradOut& o, const GsPosed& posed_args, float* gate_flags, bool pose_only);
int gs_launch_mark_visible(hipStream_t stream, int P, const float* means3D, const float* view, uint8_t* present);
// binning.hip: per-tile counts; tile scan (writes the frame's count to *num_rendered too); scatter + per-tile sort; and the
// plain exclusive scans: n counters into out[0..n], the rectangles' tile counts into off[0..P]
int gs_launch_count_tiles(hipStream_t stream, const GsFrame& f);
int gs_launch_scan_tiles(hipStream_t stream, const GsFrame& f, int32_t* num_rendered, int min_units);
int gs_launch_binning(hipStream_t stream, const GsFrame& f);
int gs_launch_scan_large(hipStream_t stream, int n, const uint32_t* in, uint32_t* out, uint32_t* block_sums, int32_t* total);
int gs_launch_scan_rect_areas(hipStream_t stream, int P, const uint2* rects, uint32_t* off, uint32_t* block_sums, int32_t* total);
// composite.hip: colour forward (train: leaves the backward's tables; `counters`: work counters or null) and backward (into the
// deterministic mode's rows when the frame has them, det_prepare / det_gather around it), frame statistics, depth and alpha maps
int gs_launch_composite_fwd(hipStream_t stream, const GsFrame& f, const float* bg, float* out_color, unsigned long long* counters,
                            bool train);
int gs_launch_composite_bwd(hipStream_t stream, const GsFrame& f, const float* bg, const float* dL_dpix, GsGrad* grads,
                            const float* out_color, unsigned long long* counters);
int gs_launch_det_prepare(hipStream_t stream, const GsFrame& f, char* det_scratch);
int gs_launch_det_gather(hipStream_t stream, const GsFrame& f, const char* det_scratch, GsGrad* grads);
int gs_launch_frame_stats(hipStream_t stream, const GsFrame& f, int64_t* stats);
int gs_launch_depth_fwd(hipStream_t stream, const GsFrame& f, float* out_depth, float* out_alpha);
int gs_launch_depth_bwd(hipStream_t stream, const GsFrame& f, const float* dL_ddepth, const float* dL_dalpha, GsGrad* grads, float* dz);
int gs_launch_depth_dz(hipStream_t stream, int P, const float* view, const float* dz, float* dL_dmeans3D);
// pose.hip, ssim.hip: what the one-call train step launches beside the frame
int gs_launch_pose_finish_partials(hipStream_t stream, const float* pose, const float* partial, int nrows, float* d_pose,
                                   float* pose_gate, const float* loss_partial, int loss_nblocks, double loss_inv_n,
                                   float lambda_dssim, float* loss, int table_rows, int table_row);
int gs_loss_fused(hipStream_t stream, int C, int H, int W, const float* img1, const float* img2, float lambda_dssim, float* dL_dimg1,
                  void* scratch);
int gs_loss_fused_nblocks(int C, int H, int W);

// projection + tile count + tile scan; stage 2 (train: leaves the backward's tables; else render-only); backward
int gs_frame_project(hipStream_t stream, const GsScene& sc, const GsView& vw, const GsFrameBufs& fb, const GsFrameCtx& cx,
                     int32_t* num_rendered, uint8_t* visible, int debug);
int gs_frame_render(hipStream_t stream, int P, const GsView& vw, const GsFrameBufs& fb, const float* bg, float* out_color, bool train,
                    int debug);
int gs_frame_backward(hipStream_t stream, const GsScene& sc, const GsView& vw, const GsFrameBufs& fb, const GsFrameCtx& cx,
                      const float* bg, const float* out_color, const float* dL_dpix, const GsGradOut& out, bool grad_scratch_is_clear,
                      int debug);

// Multi-tensor PerPointAdam (adam.hip).  `fused` (the one-call train step's launches) or null:
struct GsAdamFused {
  uint32_t* live; uint32_t seq;     // device uint32[16] persisting across steps (see k_adam_multi) and the launch's sequence number (never 0)
  // Commit gate: the frame's true instance count (gs_frame_count) and the capacity of the instance buffers, or a null count.  A
  // launch that finds count > capacity writes NOTHING — the frame dropped instances, its gradients are not the iteration's — so
  // the step can be enqueued whole, before the host has seen the count.
  const uint32_t* commit_count; unsigned long long commit_capacity;
  uint32_t* commit_poison;          // device word, sticky: set by a launch that discarded itself; later gated launches then discard themselves too
};
// With `fused`, scratch[t] is tensor t's gate flag, written by the kernels that produced the gradients.
int gs_adam_multi(hipStream_t stream, int ntensors, const int64_t* numel, const int32_t* row, float* const* params,
                  const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq, const float* const* per_point_lr,
                  const float* lr, float beta1, float beta2, float eps, const int32_t* step, float* scratch, const float* gate,
                  const int32_t* gate_index, uint32_t* live, uint32_t seq, const GsAdamFused* fused);

// ---- What the handles over a FROZEN scene share (pose tracker, camera-path renderer): the scene, the buffers of one posed frame
// carved from the caller's workspace, and that frame's arguments.
struct GsFrozenScene {
  int P, M, W, H;
  int64_t capacity;
  const float *xyz, *f_dc, *f_rest, *opacity, *scaling, *rotation;
  char *geom, *tiles, *binning;
  float *image, *consts;   // consts: identity view [16], campos [3] (gs_launch_view_consts)
  int32_t *radii, *num_rendered;   // num_rendered: where the tile scan leaves its copy of the count; the handles read count()

  // create-time checks and the scene's fields; false: refuse the handle
  bool init(int P_, int M_, int W_, int H_, int64_t capacity_, const float* xyz_, const float* f_dc_, const float* f_rest_,
            const float* opacity_, const float* scaling_, const float* rotation_, const void* workspace) {
    if (P_ <= 0 || M_ < 1 || M_ > 16 || !gs_frame_size_ok(W_, H_) || capacity_ <= 0 || !workspace) return false;
    if (!xyz_ || !f_dc_ || (M_ > 1 && !f_rest_) || !opacity_ || !scaling_ || !rotation_) return false;
    P = P_; M = M_; W = W_; H = H_; capacity = capacity_;
    xyz = xyz_; f_dc = f_dc_; f_rest = M_ > 1 ? f_rest_ : nullptr; opacity = opacity_; scaling = scaling_; rotation = rotation_;
    return true;
  }
  // train: `binning` holds the backward's tables too, laid out for `knobs`; else keys + lists only (the same for any knobs)
  void carve(GsCarver& c, const GsKnobs& knobs, bool train) {
    geom = c.take<char>(GeomLayout(P).total);
    tiles = c.take<char>(TilesLayout(W, H).total);
    binning = c.take<char>(gs_binning_bytes(capacity, W, H, knobs, train));
    image = c.take<float>(3 * (size_t)W * H);
    consts = c.take<float>(32);
    radii = c.take<int32_t>((size_t)P);
    num_rendered = c.take<int32_t>(1);
  }
  bool degree_ok(int D) const { return D >= 0 && D <= 3 && (D + 1) * (D + 1) <= M; }
  GsScene scene(int D) const {   // degree 0 reads only the DC coefficient; higher degrees read f_dc + f_rest in place
    return {P, D, D == 0 ? 1 : M, xyz, f_dc, D == 0 ? nullptr : f_rest, nullptr, opacity, scaling, rotation, nullptr, 1.0f};
  }
  GsView view(const float* proj, float tanfovx, float tanfovy) const { return {W, H, consts, proj, consts + 16, tanfovx, tanfovy}; }
  GsFrameBufs bufs(const GsKnobs& knobs, void* grad_scratch) const { return {geom, tiles, binning, capacity, radii, grad_scratch, knobs}; }
  const uint32_t* count() const { return gs_frame_count(tiles, W, H); }
};
