/*
 * mi355gs.h — C ABI of libmi355gs.so, the MI355X (gfx950 / CDNA4) implementation of the
 * InstantSplat train/render hot path.
 *
 * Boundary contract:
 *   - plain pointers, sizes and scalars only; no C++ / torch types cross this line;
 *   - every buffer (inputs, outputs, scratch) is allocated and owned by the CALLER (PyTorch's
 *     caching allocator in the Python binding); the library never allocates or frees device memory;
 *   - every kernel is enqueued on the `stream` argument (a hipStream_t passed as void*; the Python
 *     binding passes torch.cuda.current_stream().cuda_stream); calls return after enqueueing unless
 *     stated otherwise;
 *   - all floating point is fp32, all tensors contiguous and on the same device;
 *   - return value: 0 on success, a negative MI355GS_E* code otherwise (mi355gs_error_string());
 *   - state: the per-operator entry points keep nothing between calls.  Exceptions, all host-side and documented at their
 *     declarations: the opt-in event timing (mi355gs_profile_*), the process-wide tuning knob mi355gs_tune_min_units, and
 *     the trainer handle.  Threading: calls may be made from any host thread, one call at a time per stream; the
 *     composite entry points (mi355gs_posed_*, mi355gs_trainer_*, mi355gs_tracker_*, mi355gs_path_*) hand their per-call
 *     context to the shared frame functions as arguments (csrc/common.h, GsFrameCtx) — no call leaves anything behind in
 *     the library, on any thread.
 *
 * Each entry point names the reference interface it replaces. The reference's three native
 * operators are un-vendored git submodules (reference .gitmodules:1-12), so the citations are
 * to the reference's CALL SITES, which define the signatures and semantics this ABI must serve.
 */
#ifndef MI355GS_H
#define MI355GS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355GS_ABI_VERSION 10

/* error codes */
#define MI355GS_OK 0
#define MI355GS_EINVAL (-1)    /* bad argument (null pointer, non-positive size, unsupported degree) */
#define MI355GS_ELAUNCH (-2)   /* a HIP launch / runtime call failed (debug mode: which kernel is logged) */
#define MI355GS_EOVERFLOW (-3) /* instance capacity too small for this frame (see mi355gs_raster_forward_render) */

int mi355gs_abi_version(void);
const char* mi355gs_error_string(int code);

/* ------------------------------------------------------------------------------------------------
 * Differentiable Gaussian rasterizer
 * replaces: diff_gaussian_rasterization._C.rasterize_gaussians / rasterize_gaussians_backward,
 *           reached through GaussianRasterizer.forward at reference gaussian_renderer/__init__.py:126-135
 *           with the settings tuple built at gaussian_renderer/__init__.py:60-76.
 *
 * Scratch layout (caller allocates `bytes` from the *_bytes() queries, 256-byte aligned):
 *   geom    : per-Gaussian records written by preprocess, read by render and backward
 *   tiles   : per-tile counters / offsets; per-pixel final transmittance and contributor counts
 *   binning : per-instance sort keys and the depth-sorted per-tile Gaussian index lists; the backward's work units
 *             (runs of 64, 128, 256 or 512 instances of a tile's list — csrc/common.h GS_SEG, gs_unit_level_for — chosen
 *             on the device from the frame's instance count; the capacity passed to the render / backward calls bounds it) and the per-pixel state the forward leaves at their boundaries
 * The forward is split in two so the caller can size `binning` exactly (one 4-byte D2H read of
 * *num_rendered between the calls, as the reference operator does internally) or skip the read
 * and pass a capacity bound (no host sync; overflow is reported through *num_rendered > capacity).
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_raster_geom_bytes(int P);
size_t mi355gs_raster_tiles_bytes(int W, int H);
size_t mi355gs_raster_binning_bytes(int64_t num_instances, int W, int H);

/* Stage 1: per-Gaussian projection (frustum cull, EWA 2-D covariance, conic, radius, tile rect,
 * SH -> RGB), per-tile instance counts and their exclusive scan.
 *   means3D[P,3] scales[P,3] rotations[P,4] (w,x,y,z, used un-normalised) opacities[P]
 *   shs[P,M,3] (D = active degree 0..3, M = coefficients stored per Gaussian) or colors_precomp[P,3];
 *   split SH storage (the reference's own parameter layout, scene/gaussian_model.py:168-169): when shs_rest is
 *   non-null, shs is the DC coefficient [P,1,3] and shs_rest the remaining M-1 coefficients [P,M-1,3] — no
 *   cat(f_dc, f_rest) (scene/gaussian_model.py:114-117) has to be materialised
 *   cov3D_precomp[P,6] replaces scales/rotations when non-null
 *   viewmatrix[16], projmatrix[16]: row-vector convention, i.e. the transposed matrices the
 *     reference stores (scene/cameras.py:54-55) in flat memory; campos[3]
 *   radii[P] (int32, output); num_rendered: one int32 the device can write — device memory, or pinned host memory mapped into
 *   the device's address space, in which case the count reaches the host without a copy — receives the instance count R
 *   visible (ABI v7, may be null): uint8[P] (a torch.bool tensor's memory), 1 where radii > 0 — the `visibility_filter` the
 *   reference's render() computes with an elementwise kernel behind the operator (gaussian_renderer/__init__.py:142)
 *   grad_scratch (ABI v7, may be null): the mi355gs_raster_grad_scratch_bytes(P) buffer this frame's backward will be given,
 *   if the caller holds it already.  The projection kernel then clears it on its way (the per-tile counters are always
 *   cleared that way: no memset is enqueued in front of a frame), and the backward is told so: grad_scratch_is_clear = 1 */
int mi355gs_raster_forward_preprocess(
    void* stream, int P, int D, int M, int W, int H,
    const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* campos,
    float tanfovx, float tanfovy, int prefiltered,
    int32_t* radii, void* geom, void* tiles, int32_t* num_rendered, uint8_t* visible, void* grad_scratch, int debug);

/* Stage 2: scatter instances to their tiles, sort every tile's list front-to-back
 * (depth, then Gaussian index), alpha-composite.  capacity = instances `binning` was sized for.
 *   bg[3]; out_color[3,H,W] planar. */
int mi355gs_raster_forward_render(
    void* stream, int P, int W, int H, int64_t capacity, const float* bg,
    const void* geom, void* tiles, void* binning, float* out_color, int debug);

/* Stage 2 for a frame NO BACKWARD WILL FOLLOW (ABI v9) — every render under torch.no_grad(): reference render.py:87,137,177
 * (render_set, render_set_optimize's final renders, the FPS loop at :172-186), train.py:277 (training_report), evaluation.
 * Same scatter, sort and compositing, bit-identical out_color / radii / per-pixel state in `tiles`; nothing is left behind for a
 * backward: `binning` is only mi355gs_raster_binning_bytes_render_only() bytes (sort keys + the per-tile lists, 12 B per
 * instance — the training layout adds 4 KiB per 64-instance unit), and the compositing kernel's render-only instantiation stores
 * no boundary records, hit masks, unit table or quadrant maxima.  mi355gs_raster_backward must not be called on such a frame. */
size_t mi355gs_raster_binning_bytes_render_only(int64_t num_instances, int W, int H);
int mi355gs_raster_forward_render_only(
    void* stream, int P, int W, int H, int64_t capacity, const float* bg,
    const void* geom, void* tiles, void* binning, float* out_color, int debug);

/* Backward of both stages.  dL_dpix[3,H,W] in; gradients out (all written, zero where unused):
 *   dL_dmeans3D[P,3] dL_dmeans2D[P,3] (x,y in the reference's NDC-scaled screen units, z = 0)
 *   dL_dshs[P,M,3] (split storage: dL_dshs[P,1,3] + dL_dshs_rest[P,M-1,3]) or dL_dcolors[P,3], dL_dopacities[P],
 *   dL_dscales[P,3] dL_drotations[P,4] or dL_dcov3D[P,6]
 *   geom/tiles/binning/capacity/radii/out_color: exactly what the forward of this frame used and produced
 *   grad_scratch: mi355gs_raster_grad_scratch_bytes(P) bytes (per-Gaussian accumulators; the last 256 bytes, from
 *   mi355gs_raster_grad_gate_offset(P) on, are the eight gate flags mi355gs_posed_backward leaves for the optimizer)
 *   grad_scratch_is_clear (ABI v7): 1 = this frame's forward was given grad_scratch and nothing has written to it since
 *   (the backward then enqueues no memset); 0 = the backward clears it itself.  A second backward of the same frame passes 0. */
size_t mi355gs_raster_grad_scratch_bytes(int P);
size_t mi355gs_raster_grad_gate_offset(int P);
int mi355gs_raster_backward(
    void* stream, int P, int D, int M, int W, int H, const float* bg,
    const float* means3D, const float* shs, const float* shs_rest, const float* colors_precomp, const float* opacities,
    const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* campos,
    float tanfovx, float tanfovy,
    const void* geom, void* tiles, const void* binning, int64_t capacity, const int32_t* radii,
    const float* out_color, const float* dL_dpix, void* grad_scratch,
    float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dshs, float* dL_dshs_rest, float* dL_dcolors, float* dL_dopacities,
    float* dL_dscales, float* dL_drotations, float* dL_dcov3D, int grad_scratch_is_clear, int debug);

/* Depth and accumulated-alpha maps of a rendered frame, and their backward (added within ABI v10: new entry points only).
 * Per pixel, over its tile's depth-sorted list with the colour walk's own rules (csrc/composite.hip): T_i the transmittance in
 * front of entry i, alpha_i = min(0.99, opacity 2^power2), z_i the Gaussian's view depth (the z of viewmatrix applied to its
 * mean),
 *     depth = sum_i T_i alpha_i z_i   (the expected depth: NOT divided by alpha, no background term; 0 where nothing blends)
 *     alpha = 1 - final_T
 * mi355gs_raster_depth_forward runs after stage 2 of the same frame — mi355gs_raster_forward_render or
 * mi355gs_raster_forward_render_only, with the same bits after either — on its geom / tiles / binning / capacity (`binning` laid
 * out under the knobs the frame was made with; only the lists in its head are read).  out_depth[H,W], out_alpha[H,W]: either
 * may be null.  P = 0 or capacity = 0: both maps are zero.
 * mi355gs_raster_depth_backward: dL_ddepth[H,W] and dL_dalpha[H,W] in (either may be null: zero), the scene and view arguments
 * of mi355gs_raster_backward that the chain needs (colours and SH do not enter; the opacity is read from the frame's records), and
 * gradients out, all written (zero where unused): dL_dmeans3D, dL_dmeans2D, dL_dopacities, dL_dscales + dL_drotations or
 * dL_dcov3D — to be ADDED to what mi355gs_raster_backward gives for a colour gradient of the same frame.  It may follow either
 * stage 2.  depth_scratch: mi355gs_raster_depth_scratch_bytes(P) bytes, cleared by the call (per-Gaussian moment records and
 * dL/dz).  The sums are float atomics: they depend on arrival order, and mi355gs_tune_deterministic does NOT cover this call. */
int mi355gs_raster_depth_forward(
    void* stream, int P, int W, int H, int64_t capacity,
    const void* geom, const void* tiles, const void* binning, float* out_depth, float* out_alpha);
size_t mi355gs_raster_depth_scratch_bytes(int P);
int mi355gs_raster_depth_backward(
    void* stream, int P, int W, int H,
    const float* means3D, const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
    const float* viewmatrix, const float* projmatrix, const float* campos, float tanfovx, float tanfovy,
    const void* geom, const void* tiles, const void* binning, int64_t capacity, const int32_t* radii,
    const float* dL_ddepth, const float* dL_dalpha, void* depth_scratch,
    float* dL_dmeans3D, float* dL_dmeans2D, float* dL_dopacities, float* dL_dscales, float* dL_drotations, float* dL_dcov3D,
    int debug);

/* Visibility test only — replaces diff_gaussian_rasterization._C.mark_visible
 * (GaussianRasterizer.markVisible; not called by the reference's scripts). present[P] uint8. */
int mi355gs_raster_mark_visible(void* stream, int P, const float* means3D, const float* viewmatrix,
                                const float* projmatrix, uint8_t* present);

/* Frame statistics for roofline accounting (bench.py): stats[0] = R, the number of (tile, Gaussian)
 * instances of the last forward that used `tiles`; stats[1] = R_eff = sum over tiles of the largest
 * per-pixel contributor count, i.e. the instances the composite kernels actually had to consume
 * (SURVEY.md 8d).  stats: device int64[2]. */
int mi355gs_raster_frame_stats(void* stream, int W, int H, const void* tiles, int64_t* stats);

/* Tuning / test knob of the segmented backward (csrc/common.h, GS_MIN_UNITS): a frame's backward units are lengthened
 * (2, 4, 8 chunks of 64 instances) only while at least `min_units` of them remain.  Returns the previous value;
 * min_units <= 0 only queries.  Process-wide; the default (40960) is what every measurement uses — tests lower it to
 * run the multi-chunk path on small scenes.  It also enters the buffer-size queries: for the per-operator entry points set it
 * before sizing a frame's buffers and keep it until that frame's backward has been enqueued; a trainer handle takes a
 * snapshot of it at mi355gs_trainer_create and uses that for all its calls. */
int mi355gs_tune_min_units(int min_units);

/* Deterministic-backward mode (ABI v9; SURVEY.md 5 "determinism self-check").  The default backward adds the nine screen-space
 * moments of a Gaussian from every (tile, unit) that replays it with float atomics, in whatever order the waves arrive: two runs
 * of the same frame differ in the last bits, two runs of the same scene drift apart.  on = 1: every (Gaussian, tile) instance's
 * moments are stored to a row of their own and summed per Gaussian in the order of its tile rectangle (y outer, x inner) —
 * bit-identical gradients run to run, and with them bit-identical training.  Same arithmetic otherwise; costs five small
 * launches, a memset and 52 bytes per instance per backward (measured at C3: 0.84-0.87 x the default rate).
 * It enters the buffer-size queries (mi355gs_raster_binning_bytes: + 52 B per instance; mi355gs_raster_grad_scratch_bytes:
 * + ~4 B per Gaussian): set it before sizing a frame's buffers and keep it until that frame's backward has been enqueued; a
 * trainer handle takes a snapshot at mi355gs_trainer_create.  The work-counting instantiation (mi355gs_profile_work_counters)
 * is not available in this mode.  Returns the previous value; on < 0 only queries.  Process-wide. */
int mi355gs_tune_deterministic(int on);

/* Convention of dL_dscales under scale_modifier != 1 (ABI v9).  The covariance is built from s = scale_modifier * scale
 * (reference gaussian_renderer/__init__.py:29,66 is the only place the modifier comes from; it trains with 1.0).
 *   mode 0 (default): dL_dscales = dL/ds, the gradient with respect to the MODIFIED scale — what the published operator's
 *     backward returns (its computeCov3D backward forms s = mod * scale first and writes dL/ds into dL_dscale; recalled, the
 *     operator is an un-vendored submodule: reference .gitmodules:4-6).  "Results identical to the reference's" is the bar.
 *   mode 1: dL_dscales = scale_modifier * dL/ds, the true derivative with respect to `scales`.
 * The two are the same number at scale_modifier = 1.  Rotation gradients are not affected.  Returns the previous mode;
 * mode < 0 only queries.  Process-wide, read when a backward is enqueued. */
int mi355gs_tune_scale_grad(int mode);

/* Optional in-library kernel timing with HIP events recorded on the launch stream, so a caller that
 * cannot see the kernels (they are enqueued inside this library) can still attribute time to them.
 * kind: 0 = composite forward (training instantiation), 1 = composite backward, 2 = composite forward, render-only
 * instantiation, 3 = the fused L1 + SSIM loss pass (k_l1_ssim_fused), 4 = the per-tile sort (k_sort_tiles), 5 = the per-tile
 * instance count (k_count_tiles_lds).  profile_read synchronises the recorded events
 * and returns the summed milliseconds and launch count since profile_begin. */
int mi355gs_profile_begin(void);
/* Time only every `every`-th launch of a kind (default 1: all).  An event pair costs ~3.5 us of stream time, which matters when
 * the timed kernels are part of a measured loop.  Returns the previous period; every <= 0 only queries. */
int mi355gs_profile_set_period(int every);
/* While `counters` (device uint64[16], zeroed by the caller) is non-null, every composite launch runs its counting
 * instantiation and ADDS — backward: [0] (Gaussian, tile) steps, [1] quadrant bodies evaluated, [2] of those with at least one
 * valid pixel, [3] valid (pixel, Gaussian) pairs, [4] steps that ended in a reduction + atomics, [5] waves that did work;
 * forward: [8] staged 64-record groups (one cull each), [9] (Gaussian, quadrant) hits, [10] walk steps (two hits each),
 * [11] (pixel, Gaussian) pairs that pass the alpha tests, [12] of those blended (not the stopping one), [13] quadrant waves.
 * null switches back to the shipped kernels (which have no counters).  Process-wide, measurement only. */
int mi355gs_profile_work_counters(void* counters);
int mi355gs_profile_read(int kind, double* total_ms, int* launches);
int mi355gs_profile_end(void);
/* roctx ranges (ABI v10; SURVEY.md section 5, row 1: the reference has no ranges at all, its profile is TensorBoard's iter_time,
 * train.py:114-115,140,178).  While on, every entry point that enqueues kernels brackets itself with
 * roctxRangePushA(<its name>) / roctxRangePop() — the stages of a train step appear as nested ranges under
 * "mi355gs_trainer_step" in `rocprofv3 --marker-trace --kernel-trace` (tools/prof.sh).  The roctx library
 * (librocprofiler-sdk-roctx.so, else libroctx64.so) is opened with dlopen on first use: the library has no link-time dependency
 * on it, and without it this stays off.  on = 1 / 0: switch (also on at load with MI355GS_ROCTX=1); on = -1: query.
 * Returns the number of ranges pushed since the library was loaded (>= 0), or MI355GS_EINVAL if roctx could not be opened when
 * asked to switch on. */
int mi355gs_profile_ranges(int on);

/* ------------------------------------------------------------------------------------------------
 * fused SSIM (+ optional L1) loss
 * replaces: fused_ssim.fused_ssim(img1, img2) at reference train.py:173 (same value as the
 *           reference's own fallback utils/loss_utils.py:55-85: 11x11 Gaussian window, sigma 1.5,
 *           zero "same" padding, C1 = 0.01^2, C2 = 0.03^2, mean over all elements).
 *   img1, img2 [B,C,H,W]; scratch: mi355gs_ssim_scratch_bytes() bytes (per-workgroup partial sums,
 *   reduced in a fixed order so the result is run-to-run deterministic)
 *   ssim_mean / l1_mean: device float[1] each (either may be null): mean SSIM map, mean |img1-img2|
 *   dm_dmu1, dm_dsigma1_sq, dm_dsigma12 [B,C,H,W]: saved partials for backward (all null = inference)
 *   padding_valid: 0 = fused_ssim(padding="same") (the reference's use); 1 = padding="valid": the map is computed the same
 *   way but only the region where the window lies inside the image (5 px in from every edge) is averaged and passes
 *   gradient (l1_mean / l1_grad_scale must then be null; H, W > 10)
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_ssim_scratch_bytes(int B, int C, int H, int W);
int mi355gs_ssim_forward(void* stream, int B, int C, int H, int W, const float* img1, const float* img2,
                         float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                         void* scratch, float* ssim_mean, float* l1_mean, int padding_valid);
/* dL_dimg1 = ssim_grad_scale * d(ssim_mean)/dimg1 + l1_grad_scale * d(l1_mean)/dimg1
 * (scales are read from device scalars so no host sync is needed; null = 0). */
int mi355gs_ssim_backward(void* stream, int B, int C, int H, int W, const float* img1, const float* img2,
                          const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12,
                          const float* ssim_grad_scale, const float* l1_grad_scale, float* dL_dimg1, int padding_valid);
/* The reference's training loss (train.py:171-176), loss = (1 - lambda) * L1 + lambda * (1 - SSIM), and dloss_dimg1 [B,C,H,W]
 * (the gradient for dL/dloss = 1) from ONE pass over the two images: the SSIM partial-derivative maps never leave LDS, about a
 * third of the traffic of mi355gs_ssim_forward + _backward.  ssim_mean / l1_mean (optional) and loss: device float[1] each.
 * The binding's forward calls this and keeps the gradient; its backward multiplies it by the incoming dL/dloss. */
int mi355gs_l1_ssim_loss_fused(void* stream, int B, int C, int H, int W, const float* img1, const float* img2, void* scratch,
                               float lambda_dssim, float* ssim_mean, float* l1_mean, float* loss, float* dloss_dimg1);

/* ------------------------------------------------------------------------------------------------
 * l1_loss(network_output, gt) = mean |a - b| over n contiguous floats (reference utils/loss_utils.py:39-40, called at
 * train.py:171) and its gradient w.r.t. a: sgn(a - b) * (*grad_scale) / n, as autograd computes it for abs(a - b).mean()
 * (ABI v8).  scratch: mi355gs_l1_scratch_bytes(n) bytes of device memory; mean_out, grad_scale: device float[1].
 * Two launches forward (per-workgroup partial sums in float, finished in double in a fixed order), one backward.
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_l1_scratch_bytes(int64_t n);
int mi355gs_l1_loss_forward(void* stream, int64_t n, const float* a, const float* b, void* scratch, float* mean_out);
int mi355gs_l1_loss_backward(void* stream, int64_t n, const float* a, const float* b, const float* grad_scale, float* d_a);
/* ------------------------------------------------------------------------------------------------
 * The reference's loss EXPRESSION as written (ABI v9) — reference train.py:171-176:
 *     Ll1 = l1_loss(image, gt_image);  ssim_value = fused_ssim(image.unsqueeze(0), gt_image.unsqueeze(0))
 *     loss = (1.0 - opt.lambda_dssim) * Ll1 + opt.lambda_dssim * (1.0 - ssim_value);  loss.backward()
 * two operator calls on the same pair of images and four scalar operations on 0-dim tensors: sixteen eager launches
 * forward + backward.  These entry points let a binding serve that source text unmodified in three launches — TWO when the
 * backward follows the materialisation directly (program_eval_grad) —
 * (instantsplat_amd/loss_utils.py, lazy_loss.py: l1_loss runs the pair forward, fused_ssim on the same tensors takes its other half from
 * it, the scalar arithmetic is recorded on the host and evaluated by one launch, the backward of the whole expression is one
 * launch over the image).
 *   pair_forward: ONE pass over the images, one launch (the kernel of mi355gs_l1_ssim_loss_fused) -> dssim_dimg1[B,C,H,W] =
 *     d(ssim_mean)/d(img1), and both means as per-workgroup partial sums in `scratch` (mi355gs_ssim_scratch_bytes(); it must
 *     stay untouched until the last program_eval of the pair).
 *   program_eval: one launch that FINISHES the two means from `scratch` (fixed order, double accumulation: the bits
 *     mi355gs_ssim_forward / mi355gs_l1_ssim_loss_fused report) into *ssim_mean / *l1_mean (device float[1] each) and evaluates a
 *     postfix program of n_ops <= MI355GS_LOSS_PROGRAM_MAX operations over them, ops[i] / consts[i] HOST arrays, in float32 with
 *     one rounding per operation (what eager PyTorch computes for the same expression):
 *     L1 / SSIM push a mean; MULK x*k, ADDK x+k, RSUBK k-x, DIVK x*(1/k), NEG -x act on the top of the stack; ADD / SUB pop two
 *     (a b -> a+b, a-b).  *out = the one value left.  A program that underflows the stack or leaves more than one value is refused.
 *     host_out (may be null; 8-byte aligned float[2]): a second destination the DEVICE can write and the HOST can read without a
 *     copy — pinned host memory mapped into the device's address space: the kernel stores (value, ticket) there as one 8-byte
 *     store.  A caller that presets the slot and polls for its ticket has the value as soon as this launch has run — reference
 *     train.py:188 `loss.item()` then neither enqueues a copy nor waits for the backward kernels queued behind the loss.
 *   pair_backward: d_img1[n] = ((g_l1 ? *g_l1 : 1) * c_l1 / n) * sgn(img1 - img2) + ((g_ssim ? *g_ssim : 1) * c_ssim) * dssim_dimg1
 *     — the gradient of  c_l1 * l1_mean + c_ssim * ssim_mean  scaled by incoming gradients read from device scalars (autograd's own
 *     operation order for abs(a - b).mean()); dssim_dimg1 may be null when c_ssim == 0.
 * ---------------------------------------------------------------------------------------------- */
#define MI355GS_LOSS_PROGRAM_MAX 16
#define MI355GS_LOSS_OP_L1 0
#define MI355GS_LOSS_OP_SSIM 1
#define MI355GS_LOSS_OP_MULK 2
#define MI355GS_LOSS_OP_ADDK 3
#define MI355GS_LOSS_OP_RSUBK 4
#define MI355GS_LOSS_OP_DIVK 5
#define MI355GS_LOSS_OP_NEG 6
#define MI355GS_LOSS_OP_ADD 7
#define MI355GS_LOSS_OP_SUB 8
int mi355gs_l1_ssim_pair_forward(void* stream, int B, int C, int H, int W, const float* img1, const float* img2, void* scratch,
                                 float* dssim_dimg1);
int mi355gs_l1_ssim_pair_backward(void* stream, int64_t n, const float* img1, const float* img2, const float* dssim_dimg1,
                                  const float* g_l1, float c_l1, const float* g_ssim, float c_ssim, float* d_img1);
int mi355gs_loss_program_eval(void* stream, int n_ops, const int32_t* ops, const float* consts, int B, int C, int H, int W,
                              const void* scratch, float* ssim_mean, float* l1_mean, float* out, float* host_out, float ticket);
/* program_eval AND pair_backward for dL/d(value) = 1 in ONE launch (g_l1 = g_ssim = 1; c_l1 / c_ssim: the partial derivatives of
 * the program with respect to the two means): what `loss.backward()` right behind the materialisation needs — the gradient over
 * the image does not depend on the means, so one workgroup finishes the value while the others write d_img1[B*C*H*W]. */
int mi355gs_loss_program_eval_grad(void* stream, int n_ops, const int32_t* ops, const float* consts, int B, int C, int H, int W,
                                   const void* scratch, float* ssim_mean, float* l1_mean, float* out, float* host_out, float ticket,
                                   const float* img1, const float* img2, const float* dssim_dimg1, float c_l1, float c_ssim, float* d_img1);

/* ------------------------------------------------------------------------------------------------
 * simple-knn
 * replaces: simple_knn._C.distCUDA2(points) at reference scene/gaussian_model.py:156 —
 *           mean of the squared distances to the 3 nearest other points (exact).
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_knn_scratch_bytes(int N);
int mi355gs_knn_dist2(void* stream, int N, const float* points, float* mean_dist2, void* scratch);

/* ------------------------------------------------------------------------------------------------
 * per-point Adam
 * replaces: PerPointAdam.step at reference scene/per_point_adam.py:34-100 for one parameter tensor
 *   n = elements, row = elements per point (per_point_lr has n/row entries, or null)
 *   grad_sumsq: device float[1] holding sum(grad^2) — the reference gates the moment update on the
 *   whole-tensor norm being > 0 (per_point_adam.py:62-69); pass null to always update.
 * ---------------------------------------------------------------------------------------------- */
int mi355gs_adam_step(void* stream, int64_t n, int row, float* param, const float* grad, float* exp_avg,
                      float* exp_avg_sq, const float* per_point_lr, const float* grad_sumsq,
                      float lr, float beta1, float beta2, float eps, int step);

/* All parameter tensors of one optimizer step in two launches (<= 8 tensors per call).  The arrays are
 * HOST arrays of length ntensors holding device pointers / per-tensor scalars; per_point_lr[t] may be null;
 * step[t] is the 1-based step count of tensor t; scratch: device float[8].  The whole-tensor gradient gate
 * of the reference (per_point_adam.py:62-69) is evaluated on the device from the summed squares — or, when `gate` is
 * non-null, taken from flags the gradients' producer has already left on the device: tensor t updates its moments iff
 * gate[gate_index[t]] > 0 (device float[8] / host int32[ntensors], entries 0..7; `scratch` may then be null) and the
 * pass over all gradients is not launched.  mi355gs_posed_backward leaves such flags behind its gradient records
 * (group order xyz, f_dc, f_rest, opacity, scaling, rotation, pose); the caller vouches that grads[t] is exactly the
 * tensor that call wrote.
 * live / seq (ABI v7, live may be null): a memory of gated-off tensors ACROSS calls, owned by the caller — device uint32[16],
 * zeroed once, handed to every step of the same tensor list together with a sequence number that differs from call to call
 * and is never 0.  A tensor whose gradient is all zero keeps its moments and takes the parameter step p - s * (m / denom),
 * which is the identity wherever the first moment is zero; a call that scanned such a tensor completely without meeting a
 * non-zero first moment says so in `live`, and later calls skip the tensor without reading anything (f_rest before the SH
 * degree is raised: 4 B per element per step otherwise).  Any update of the tensor resets its entry.  The caller must zero
 * `live` again if anything but these calls writes the moments. */
int mi355gs_adam_multi_step(void* stream, int ntensors, const int64_t* numel, const int32_t* row, float* const* params,
                            const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                            const float* const* per_point_lr, const float* lr, float beta1, float beta2, float eps,
                            const int32_t* step, float* scratch, const float* gate, const int32_t* gate_index,
                            uint32_t* live, uint32_t seq);

/* ------------------------------------------------------------------------------------------------
 * InstantSplat camera-frame transform fused with the Gaussian activations
 * replaces: the PyTorch ops of reference gaussian_renderer/__init__.py:81-103 —
 *   rel_w2c = get_camera_from_tensor(pose) (utils/pose_utils.py:57-84, quaternion normalised),
 *   means_cam = rel_w2c @ [xyz,1], rot_cam = quadmultiply(pose[:4], rotation) (raw quaternions),
 *   opacity = sigmoid(_opacity), scales = exp(_scaling) (scene/gaussian_model.py:101-124) — and their
 *   autograd backward, including the reduction over all Gaussians to dL/dpose[7].
 *   pose[7] = (qw,qx,qy,qz,tx,ty,tz) on the device; scratch: device float[32] (16 sums, a ticket counter, padding).
 * ---------------------------------------------------------------------------------------------- */
int mi355gs_pose_forward(void* stream, int P, const float* xyz, const float* rot, const float* scaling,
                         const float* opacity_logit, const float* pose, float* means_cam, float* rot_cam, float* scales,
                         float* opac);
int mi355gs_pose_backward(void* stream, int P, const float* xyz, const float* rot, const float* scales, const float* opac,
                          const float* pose, const float* g_means, const float* g_rot, const float* g_scales,
                          const float* g_opac, float* d_xyz, float* d_rot, float* d_scaling, float* d_opacity_logit,
                          float* d_pose, float* scratch);

/* ------------------------------------------------------------------------------------------------
 * InstantSplat's render() as the operator sees it: Gaussians in the WORLD frame with RAW parameters plus the learnable
 * camera pose — the projection kernels apply the camera-frame transform and the activations themselves, and their backward
 * goes all the way to the raw-parameter gradients and dL/dpose[7]: no camera-frame intermediates in HBM, three launches fewer
 * per iteration than mi355gs_pose_forward + mi355gs_raster_* + mi355gs_pose_backward, ONE autograd node in the binding.
 * replaces: everything reference gaussian_renderer/__init__.py:81-135 does between the GaussianModel and the image for the
 *   default pipeline (SH colours, scale/rotation covariance): get_camera_from_tensor, the [4,4]@[4,P] transform,
 *   quadmultiply, sigmoid / exp, cat(f_dc, f_rest), GaussianRasterizer.forward — and their autograd.
 *   xyz[P,3], f_dc[P,1,3], f_rest[P,15,3] (may be null while D == 0: only the DC coefficient is read), opacity_logit[P,1],
 *   log_scales[P,3], rotation[P,4] raw (w,x,y,z), pose[7] = (qw,qx,qy,qz,tx,ty,tz), all on the device.
 *   view_identity[16] / origin[3]: device constants (identity matrix, zeros) — InstantSplat hands the operator an
 *   identity view and a camera at the origin (reference :55-59); kept as arguments because the library owns no memory.
 *   Stage 2 of the forward is mi355gs_raster_forward_render, unchanged.  visible / grad_scratch / grad_scratch_is_clear: as for
 *   mi355gs_raster_forward_preprocess / _backward.
 *   backward: pose_scratch = device float[16 * ((P + 255) / 256) + 32]; d_f_rest may be null while D == 0 (the reference's
 *   gradient for it is all zero then); d_* receive dL/d(raw parameter), d_pose[7] dL/dpose.
 *   pose_rows / pose_row (ABI v8): with pose_rows > 0, d_pose is the gradient of the WHOLE pose table the 7-vector was taken
 *   from — float[pose_rows, 7] (reference scene/gaussian_model.py:134-136, `P[idx]`): row pose_row receives dL/dpose and every
 *   other row is written 0, which is what autograd's backward of the row selection builds with a fill and a copy of its own.
 *   pose_rows == 0: d_pose[7] as before.
 *   Also written: PerPointAdam's whole-tensor gate flags for these gradients, float[8] at grad_scratch +
 *   mi355gs_raster_grad_gate_offset(P): flag k > 0 <=> the gradient of group k (xyz, f_dc, f_rest, opacity, scaling,
 *   rotation, pose) has a non-zero element — what mi355gs_adam_multi_step(gate=...) consumes instead of re-reading them.
 * ---------------------------------------------------------------------------------------------- */
int mi355gs_posed_forward_preprocess(void* stream, int P, int D, int W, int H, const float* xyz, const float* f_dc,
                                     const float* f_rest, const float* opacity_logit, const float* log_scales, float scale_modifier,
                                     const float* rotation, const float* pose, const float* view_identity, const float* projmatrix,
                                     const float* origin, float tanfovx, float tanfovy, int32_t* radii, void* geom, void* tiles,
                                     int32_t* num_rendered, uint8_t* visible, void* grad_scratch, int debug);
int mi355gs_posed_backward(void* stream, int P, int D, int W, int H, const float* bg, const float* xyz, const float* f_dc,
                           const float* f_rest, const float* opacity_logit, const float* log_scales, float scale_modifier,
                           const float* rotation, const float* pose, const float* view_identity, const float* projmatrix,
                           const float* origin, float tanfovx, float tanfovy, const void* geom, void* tiles, const void* binning,
                           int64_t capacity, const int32_t* radii, const float* out_color, const float* dL_dpix,
                           void* grad_scratch, float* pose_scratch, float* d_xyz, float* d_means2D, float* d_f_dc, float* d_f_rest,
                           float* d_opacity_logit, float* d_log_scales, float* d_rotation, float* d_pose, int pose_rows, int pose_row,
                           int grad_scratch_is_clear, int debug);

/* ------------------------------------------------------------------------------------------------
 * Whole train iteration in one call
 * replaces: the body of the loop at reference train.py:140-211 — render(camera_pose=P[view]) -> (1-l)*L1 +
 *   l*(1-SSIM) -> backward -> PerPointAdam.step() — for the configuration the reference's scripts run: SH colours
 *   (active degree sh_degree 0..3 over 16 stored coefficients), scale/rotation covariance, --pp_optimizer
 *   --optim_pose.  11 launches, no host sync.
 *   Parameter tensors use the reference's GaussianModel layouts (scene/gaussian_model.py:166-171): xyz[P,3],
 *   f_dc[P,1,3], f_rest[P,15,3], opacity[P,1], scaling[P,3], rotation[P,4], poses[V,7]; exp_avg/exp_avg_sq: host
 *   arrays of 7 device pointers in the optimizer's group order (xyz, f_dc, f_rest, opacity, scaling, rotation, pose).
 *   workspace: mi355gs_trainer_workspace_bytes() bytes, owned by the caller, must outlive the handle.
 *   The handle is the only writer of the parameter and moment tensors while it is alive (it remembers across steps that
 *   a tensor without gradients has an all-zero first moment and then skips it; create a new handle after changing them).
 *   capacity: instance capacity of the binning buffers; *num_rendered (device-writable, see above) receives the true count of every
 *   step — a step with num_rendered > capacity dropped instances and must be discarded by the caller.  With
 *   do_optimizer_step = 1 the optimizer launch of such a step discards ITSELF: it reads the count and the capacity on the
 *   device and writes no parameter and no moment when the count is larger (commit gate), so the whole iteration can be enqueued
 *   before the host has seen the count and an overflowed one is simply repeated with larger buffers; its loss_out / gradients are
 *   those of the truncated frame.  The gate is STICKY (ABI v8): once a step of a handle has discarded itself, every later
 *   do_optimizer_step = 1 step of that handle discards itself too, whatever its own count — so a caller that enqueues many steps
 *   ahead of its reads of the counts finds parameters and moments exactly as the last step BEFORE the first overflow left them,
 *   needs no snapshot to return to, and continues from there with larger buffers, i.e. a new handle (ABI v9 dropped
 *   mi355gs_trainer_rearm: no caller keeps a handle whose buffers a frame has outgrown).  (mi355gs_trainer_optimizer_step, below,
 *   is gated only if asked to be.)
 *   lr[7], step[7] (1-based Adam step of each group): host arrays.  loss_out: device float[1].
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_trainer_workspace_bytes(int P, int W, int H, int V, int64_t capacity);
void* mi355gs_trainer_create(int P, int W, int H, int V, int64_t capacity, float* xyz, float* f_dc, float* f_rest, float* opacity,
                             float* scaling, float* rotation, float* poses, float* const* exp_avg, float* const* exp_avg_sq,
                             const float* per_point_lr, void* workspace);
int mi355gs_trainer_step(void* trainer, void* stream, int view, int sh_degree, const float* gt_image, const float* projmatrix,
                         float tanfovx, float tanfovy, const float* bg, const float* lr, const int32_t* step, float beta1, float beta2, float eps,
                         float lambda_dssim, int do_optimizer_step, float* loss_out, int32_t* num_rendered_out);
/* PerPointAdam over all 7 groups with the gradients left by the last mi355gs_trainer_step(..., do_optimizer_step = 0):
 * lets a caller inspect the loss / instance count of an iteration before committing its update (commit_gate = 0: the caller's
 * own decision, not gated) — or, commit_gate = 1 (ABI v8), split an iteration in two enqueues without having seen the count:
 * the launch then carries the same sticky device-side gate as a do_optimizer_step = 1 step, on the count of the frame whose
 * gradients it applies.  (What that buys: forward + backward of iteration t + 1 can be enqueued BEFORE the host reads the loss
 * of iteration t, its update after — the device never waits for the host and the host still sees every loss.) */
int mi355gs_trainer_optimizer_step(void* trainer, void* stream, const float* lr, const int32_t* step, float beta1, float beta2,
                                   float eps, int commit_gate);
void mi355gs_trainer_destroy(void* trainer);
/* Device pointer of the gradient buffer of parameter group k (0..6: xyz, f_dc, f_rest, opacity, scaling, rotation, poses)
 * as left by the last mi355gs_trainer_step — for tests and diagnostics (gradient parity of the fused step). */
const float* mi355gs_trainer_grad(void* trainer, int k);

/* ----------------------------------------------------------------------------------------------
 * Test-view pose tracking (reference render.py:99-170, `render_set_optimize`): Gaussians frozen, one 7-vector camera pose
 * (qw,qx,qy,qz,tx,ty,tz) optimised per view by masked L1 (mask = render > 0), torch's Adam (betas 0.9/0.999, eps 1e-8,
 * L2 weight decay 1e-4; lr 3e-3 for t, 1e-3 for the raw quaternion, cosine-annealed) and keep-best.  One iteration is the
 * posed projection, binning and composite forward, one masked-L1 value + gradient launch, the composite backward, a
 * pose-only projection backward (no per-Gaussian gradient is stored) and one single-workgroup finish that sums the
 * partials, steps Adam and keeps the best pose.  No host synchronisation inside mi355gs_tracker_run.
 *
 *   create: raw Gaussian parameters (read only; f_dc [P,3], f_rest [P,M-1,3] or null when M == 1), the fixed image size and
 *   instance capacity; workspace: mi355gs_tracker_workspace_bytes() bytes, owned by the caller.  The deterministic-backward
 *   and unit-length knobs are pinned at create.  Nothing allocates.
 *   state: caller-owned device float[MI355GS_TRACKER_STATE_FLOATS], initialised by the caller (pose and candidate = the
 *   initial pose, moments 0, best 1e20, initial loss NaN, flag and count 0); see the offsets below.
 *   sched: device float[num_iter][4] per iteration i (0-based): -lr_t(i)/(1-0.9^(i+1)), -lr_q(i)/(1-0.9^(i+1)),
 *   sqrt(1-0.999^(i+1)), unused — each computed in double and rounded to float once.
 *   run: enqueues iterations first_iter .. first_iter+n_iters-1.  pose_trace [num_iter][7] (the pose each render used),
 *   loss_trace [num_iter] and grad_trace [num_iter][7] (d loss / d pose) are optional (null) and indexed by iteration.
 *   Overflow: an iteration whose instance count exceeds the capacity sets the sticky flag; it and every later iteration of
 *   that state leave pose, moments, best and candidate unchanged.  The count slot holds the largest count seen.
 *   count: the exact instance count at `pose` (device float[7]) into *count_out (device int32), for sizing the capacity.
 *   Streams: a tracker (and a trainer) handle writes its identity view / zero camera position once, on the stream of its first
 *   call; use a handle on ONE stream, or order its first call before calls on another.
 * ---------------------------------------------------------------------------------------------- */
#define MI355GS_TRACKER_STATE_FLOATS 40
#define MI355GS_TRACKER_POSE 0        /* [7] current pose */
#define MI355GS_TRACKER_EXP_AVG 8     /* [7] */
#define MI355GS_TRACKER_EXP_AVG_SQ 16 /* [7] */
#define MI355GS_TRACKER_BEST 24       /* best loss so far */
#define MI355GS_TRACKER_INITIAL 25    /* loss of iteration 0 */
#define MI355GS_TRACKER_FLAG 26       /* uint32: sticky capacity-overflow flag */
#define MI355GS_TRACKER_COUNT 27      /* uint32: largest instance count seen */
#define MI355GS_TRACKER_CAND 32       /* [7] best pose (the pose after the step of the best iteration) */
size_t mi355gs_tracker_workspace_bytes(int P, int W, int H, int64_t capacity);
void* mi355gs_tracker_create(int P, int M, int W, int H, int64_t capacity, const float* xyz, const float* f_dc, const float* f_rest,
                             const float* opacity, const float* scaling, const float* rotation, void* workspace);
int mi355gs_tracker_count(void* tracker, void* stream, int sh_degree, const float* projmatrix, float tanfovx, float tanfovy,
                          const float* pose, int32_t* count_out);
int mi355gs_tracker_run(void* tracker, void* stream, int sh_degree, const float* gt_image, const float* projmatrix, float tanfovx,
                        float tanfovy, const float* bg, const float* sched, int num_iter, int first_iter, int n_iters, float* state,
                        float* pose_trace, float* loss_trace, float* grad_trace);
void mi355gs_tracker_destroy(void* tracker);

/* ----------------------------------------------------------------------------------------------
 * Camera paths (reference render.py:78-97, `render_set`, and its --infer_video stage :233-248): a list of poses rendered to
 * 8-bit frames with the Gaussians frozen and no gradient.
 *
 *   rgb8_from_planar: img [3,H,W] float -> out [H,W,3] uint8 with the arithmetic of torchvision.utils.save_image
 *   (x.mul(255).add_(0.5).clamp_(0, 255).to(uint8): an fp32 multiply and an fp32 add, each rounded once, clamp, truncation);
 *   a NaN gives 0.  out: device memory or pinned host memory mapped into the device's address space.  One launch.
 *
 *   path handle, shaped like the tracker's: raw Gaussian parameters (read only; f_dc [P,3], f_rest [P,M-1,3] or null when
 *   M == 1), the fixed image size and instance capacity; workspace: mi355gs_path_workspace_bytes() bytes, owned by the caller
 *   (projection records, tile tables, the render-only binning buffer, radii, one [3,H,W] float image).  Nothing allocates.
 *   render: enqueues, for every pose i of first .. first+n-1 of poses (device float[N][7], (qw,qx,qy,qz,tx,ty,tz)), the posed
 *   projection, the binning and the render-only compositing at the handle's capacity, and one launch that converts the image
 *   into frames + i*H*W*3 (uint8 [N][H][W][3]; device memory or mapped pinned host memory) and copies the frame's true instance
 *   count to counts[i] (device int32[N]): 7 launches per frame (and one 2 us launch per call that writes the handle's identity
 *   view / zero camera position on the call's stream, so a handle may be used on any stream, one call at a time), no memset, no
 *   host synchronisation, no event, no copy.
 *   Slots outside the range are not touched.  Frame i is valid exactly when counts[i] <= capacity; an overflowed frame holds
 *   the truncated render of mi355gs_raster_forward_render_only.  Overflow is per frame, not sticky: frames are independent.
 * ---------------------------------------------------------------------------------------------- */
int mi355gs_rgb8_from_planar(void* stream, int H, int W, const float* img, uint8_t* out);
size_t mi355gs_path_workspace_bytes(int P, int W, int H, int64_t capacity);
void* mi355gs_path_create(int P, int M, int W, int H, int64_t capacity, const float* xyz, const float* f_dc, const float* f_rest,
                          const float* opacity, const float* scaling, const float* rotation, void* workspace);
int mi355gs_path_render(void* path, void* stream, int sh_degree, const float* projmatrix, float tanfovx, float tanfovy,
                        const float* bg, const float* poses, int first, int n, uint8_t* frames, int32_t* counts);
void mi355gs_path_destroy(void* path);

/* ----------------------------------------------------------------------------------------------
 * Evaluation of 8-bit frame sets (reference metrics.py:60-70 on the images utils/sfm_utils.py:452-462 `readImages` loads):
 * a, b: N pairs of interleaved frames, uint8 [N][H][W][3] each, in device memory (no alignment is required of the bases:
 * a slice of a stack of odd-sized frames is fine).  Per pair i
 *   sq_sum[i]    = sum over the 3 H W byte pairs of (a - b)^2, an exact integer (32-bit partial sums per workgroup, finished
 *                  in 64 bits): psnr's mse (utils/image_utils.py:17-19) is sq_sum / (65025 * 3 H W);
 *   ssim_mean[i] = utils/loss_utils.py:55-85 `ssim` of the pair as torchvision's to_tensor hands it over: x = byte / 255 as a
 *                  correctly rounded fp32 quotient, 11x11 Gaussian window (sigma 1.5), zero "same" padding, C1 = 0.01^2,
 *                  C2 = 0.03^2, mean over 3 H W (float partial sums per workgroup, finished per pair in a fixed order in double).
 *                  A window whose moments are bit-equal in both frames counts exactly 1: identical pairs, all-black ones
 *                  included, give sq_sum = 0 and ssim_mean = 1.0f exactly.
 * Two launches per call whatever N is (one over all 32x16 tiles of all pairs, 6 bytes read per pixel pair, and one finishing
 * launch), on the caller's stream; no host synchronisation, no allocation, no memset.  scratch: the scratch-size query's bytes of
 * device memory, owned by the caller (0 = the sizes are refused).  sq_sum, ssim_mean: device arrays of N.
 * Limits (MI355GS_EINVAL beyond them, as for null pointers and non-positive sizes): N <= 65535, H <= 1048560,
 * 3 H W <= 2^31 - 1 (a byte's offset inside a frame is an int), N x ceil(H / 16) x ceil(W / 32) <= 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_metrics_rgb8_scratch_bytes(int N, int H, int W);
int mi355gs_metrics_rgb8(void* stream, int N, int H, int W, const uint8_t* a, const uint8_t* b, void* scratch, int64_t* sq_sum,
                         float* ssim_mean);

/* ----------------------------------------------------------------------------------------------
 * LPIPS with the VGG16 trunk (csrc/lpips.hip; reference lpipsPyTorch/modules/{lpips,networks,utils}.py as metrics.py:69 calls
 * it).  a, b: N pairs of interleaved frames, uint8 [N][H][W][3] each, in device memory, any base address.  Per pair:
 *   x = (byte / 255 - mean) / std in float32, mean (-.030, -.088, -.188), std (.458, .448, .450) — NO rescaling to [-1, 1],
 *   as the reference feeds `to_tensor` images; five blocks of 2, 2, 3, 3, 3 convolutions (3x3, zero padding 1, bias, ReLU),
 *   a 2x2 stride-2 max-pool (floor) in front of blocks 2 to 5, block b of width channels[b] (every multiple of 32 from 32 to
 *   512; the trained net is 64, 128, 256, 512, 512); behind each block's last ReLU a tap:
 *   n = sqrt(sum_c x_c^2), x^ = x / (n + 1e-10), d = sum_c lin_c (x^_c - y^_c)^2, tap value = mean of d over the block's pixels;
 *   taps[i][0..4] = the five tap values (taps may be NULL), lpips[i] = their sum.
 * Exact float32 throughout: every convolution is a k-ordered fused-multiply-add chain (v_mfma_f32_32x32x2_f32; the first layer on
 * the vector unit), k = (3 ky + kx) Cin + ci, started at 0, the bias added last.  No atomics: equal bits run to run and under
 * an exchange of a and b; identical frames give exactly 0.
 * weights: ONE device blob of floats, 16-byte aligned: for each of the 13 convolutions in network order the matrix
 *   [9 Cin][Cout] (row (3 ky + kx) Cin + ci, i.e. torch's weight.permute(2, 3, 1, 0)) followed by the bias [Cout]; then the five
 *   lin vectors [channels[b]] (signed values allowed).  Cin of the first convolution is 3.
 * Launches: 13 convolutions, 4 pools, 5 taps, 1 finish, on the caller's stream; no host synchronisation, no allocation, no
 * memset.  scratch: the scratch-size query's bytes of device memory, 16-byte aligned, owned by the caller: two activation
 * buffers of max_b(2 N H_b W_b channels[b]) floats and the taps' partial sums (0 = the sizes are refused).
 * Limits (MI355GS_EINVAL beyond them, as for null a, b, channels, weights, scratch or lpips and misaligned weights or scratch):
 * H, W >= 16 (block 5 needs one pixel), N <= 65535, 3 H W <= 2^31 - 1, 2 N H_b W_b channels[b] <= 2^31 - 1 for every block b
 * (an activation's element index is an int; callers split N), channels[b] a multiple of 32 in [32, 512].
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_lpips_vgg_scratch_bytes(int N, int H, int W, const int channels[5]);
int mi355gs_lpips_vgg_rgb8(void* stream, int N, int H, int W, const uint8_t* a, const uint8_t* b, const int channels[5],
                           const float* weights, void* scratch, float* lpips, float* taps);

/* ----------------------------------------------------------------------------------------------
 * MASt3R's transformer trunk (csrc/vit.hip; reference dust3r/model.py:127-190 for the wiring, the published croco blocks for
 * the arithmetic): a ViT encoder over 16 x 16 patches, decoder_embed, and two decoders whose blocks cross-attend to each other's
 * previous-layer output.  float32 throughout; every linear layer is a k-ordered fused-multiply-add chain
 * (v_mfma_f32_32x32x2_f32), started at 0, the bias added last.  No atomics: equal bits run to run, and a token's result does not
 * depend on how many images or edges share the call.
 *   block(x):        x += proj(attention(qkv(norm1(x))));  x += fc2(gelu(fc1(norm2(x))))            (GELU: exact erf)
 *   dec_block(x, y): x += proj(attention(qkv(norm1(x))));  x += cproj(attention(projq(norm2(x)), projk(norm_y(y)), projv(norm_y(y))));
 *                    x += fc2(gelu(fc1(norm3(x))))
 *   LayerNorm: eps 1e-6, biased variance.  attention: heads of 64 channels, q and k turned by RoPE2D (the first 32 channels of a
 *   head by the token's grid row, the last 32 by its column; channel j of a half pairs with j +- 16), softmax(q k^T / 8) v.
 *   Token n of an image sits at row n / Wt, column n % Wt of the Ht x Wt grid.
 * cfg: the sizes.  hooks: hooks[0] = 0 < hooks[1] < hooks[2] < hooks[3] = dec_depth — the decoder layers whose outputs a head reads.
 * weights: ONE device blob of floats, 16-byte aligned; a linear layer [K -> N] is the matrix [K][N] (torch's weight transposed)
 *   followed by its bias [N], a LayerNorm its weight [D] then its bias [D].  In order:
 *     patch embedding [768 -> enc_dim] (row (c 16 + py) 16 + px: torch's convolution weight flattened, transposed);
 *     enc_depth blocks of: norm1, qkv [D -> 3D] (column which D + head 64 + d), proj [D -> D], norm2, fc1 [D -> 4D], fc2 [4D -> D];
 *     enc_norm; decoder_embed [enc_dim -> dec_dim];
 *     dec_depth blocks of side 1, then dec_depth blocks of side 2, each: norm1, qkv, proj, norm_y, norm2, projq, projk, projv,
 *     cross proj (four [D -> D]), norm3, fc1, fc2;  dec_norm.
 * rope: device floats, cos [P][16] then sin [P][16], P = max(Ht, Wt): cos / sin of p base^(-2 i / 32), i = 0..15 (the caller
 *   builds it once per grid; MASt3R's base is 100).
 * mi355gs_vit_encode: images float32 planar [V][3][16 Ht][16 Wt] -> feat [V][Ht Wt][enc_dim] (after enc_norm).
 * mi355gs_vit_decode: feat as above and E directed edges (i, j), int32 [E][2] in HOST memory: checked against V, then copied
 *   into the scratch with hipMemcpyAsync on the stream.  From pageable memory the runtime has taken the bytes when the call
 *   returns (the caller may free them then), and MAY make the host wait for the stream's earlier work to do so — the one place
 *   where a call can block; pinned memory is copied when the stream reaches the copy and must stay valid until then.
 *   -> per side four tensors: out1[0] = feat of image i per edge, [E][Ht Wt][enc_dim]; out1[1..2] = side
 *   1 after decoder layers hooks[1], hooks[2]; out1[3] = dec_norm of side 1 after the last layer, [E][Ht Wt][dec_dim] each; out2
 *   likewise for image j and side 2.  Side 1 of layer l reads (side 1, side 2) of layer l - 1, side 2 reads (side 2, side 1).
 * scratch: the query's bytes of device memory, 16-byte aligned, owned by the caller (0 = the sizes are refused).  Launches on the
 * caller's stream; no allocation, no memset, and no host synchronisation of the library's own (decode's edge copy: above).
 * Limits (MI355GS_EINVAL beyond them, as for null pointers and weights, images, feat, scratch or outputs off a 16-byte boundary):
 * enc_dim, dec_dim multiples of 64 in [64, 1024]; heads x 64 = width; depths in [1, 256]; patch = 16; Ht Wt <= 4096; V <= 256;
 * E <= 65535; every edge index in [0, V).
 * ---------------------------------------------------------------------------------------------- */
typedef struct mi355gs_vit_config {
  int enc_dim, enc_depth, enc_heads;
  int dec_dim, dec_depth, dec_heads;
  int patch;
  int hooks[4];
} mi355gs_vit_config;
size_t mi355gs_vit_encode_scratch_bytes(const mi355gs_vit_config* cfg, int Ht, int Wt, int V);
int mi355gs_vit_encode(void* stream, const mi355gs_vit_config* cfg, const float* weights, const float* rope, int Ht, int Wt, int V,
                       const float* images, void* scratch, float* feat);
size_t mi355gs_vit_decode_scratch_bytes(const mi355gs_vit_config* cfg, int Ht, int Wt, int E);
int mi355gs_vit_decode(void* stream, const mi355gs_vit_config* cfg, const float* weights, const float* rope, int Ht, int Wt, int V, int E,
                       const int32_t* edges, const float* feat, void* scratch, float* const out1[4], float* const out2[4]);

/* ----------------------------------------------------------------------------------------------
 * MASt3R's dense heads (csrc/dpt.hip): what turns mi355gs_vit_decode's four hooked tensors of one side into that side's output.
 * The order of operations is dust3r/heads/dpt_head.py's and mast3r/catmlp_dpt_head.py's; the block definitions (croco's DPT
 * adapter, its ResidualConvUnit and FeatureFusionBlock, its Mlp) are the published ones, recalled.  float32 throughout,
 * activations channels-last; every product is a k-ordered fused-multiply-add chain (v_mfma_f32_32x32x2_f32) started at 0, the bias
 * added last, a residual after the bias.  No atomics: equal bits run to run, and a pixel's result does not depend on how many
 * edges share the call.
 *
 * mi355gs_dpt_head, on a grid of Ht x Wt tokens (H = 16 Ht, W = 16 Wt; token n at row n / Wt, column n % Wt):
 *   act_postprocess[k] on hooks[k] [E][Ht Wt][dim_tokens[k]]:
 *     k = 0: 1x1 -> layer_dims[0], ConvTranspose kernel 4 stride 4 (4 Ht x 4 Wt);  k = 1: 1x1 -> layer_dims[1], ConvTranspose kernel 2
 *     stride 2;  k = 2: 1x1 -> layer_dims[2];  k = 3: 1x1 -> layer_dims[3], 3x3 stride 2 padding 1 (ceil(Ht / 2) x ceil(Wt / 2))
 *   L[k] = layer_rn[k]: 3x3, padding 1, layer_dims[k] -> F = feature_dim, no bias
 *   rcu(x) = x + conv2(relu(conv1(relu(x))))  (3x3, F -> F, bias; the skip adds the un-rectified x)
 *   fusion(a[, b]) = out_conv(up2(rcu2(a [+ rcu1(b)])))  (up2: bilinear x 2, align_corners; out_conv 1x1 F -> F)
 *   path_4 = fusion4(L[3]) cropped to L[2]'s size; path_3 = fusion3(path_4, L[2]); path_2 = fusion2(path_3, L[1]);
 *   path_1 = fusion1(path_2, L[0])  (8 Ht x 8 Wt)
 *   head: 3x3 F -> F / 2, up2 (H x W), 3x3 F / 2 -> last_dim, ReLU, 1x1 last_dim -> 4 = (x, y, z, c)
 *   postprocess: d = |xyz|, pts3d = xyz / max(d, 1e-8) * expm1(d);  conf = conf_vmin + min(exp(c), conf_vmax - conf_vmin)
 *   -> pts3d [E][H][W][3], conf [E][H][W]; raw4 (may be NULL; 16-byte aligned) [E][H][W][4] = (x, y, z, c).
 *   The last_dim-channel tensor never reaches memory: ReLU, the 1x1 and postprocess run in the last convolution's epilogue.
 * weights of a head: ONE device blob of floats, 16-byte aligned.  A 1x1 convolution or linear layer [K -> N] is the matrix [K][N]
 * followed by its bias [N]; a 3x3 convolution [9 Cin][Cout], row (3 ky + kx) Cin + ci (torch's weight.permute(2, 3, 1, 0)), followed
 * by its bias where it has one; a ConvTranspose of stride s [C][s s C], column (dy s + dx) C + co (torch's weight.permute(0, 2, 3, 1)),
 * followed by its bias repeated s s times.  In order:
 *   act_postprocess: 0.0, 0.1 (transpose), 1.0, 1.1 (transpose), 2.0, 3.0, 3.1 (3x3);  layer_rn 0..3 (no bias);
 *   refinenet4: resConfUnit2.conv1, .conv2, out_conv;  refinenet3, 2, 1 each: resConfUnit1.conv1, .conv2, resConfUnit2.conv1, .conv2,
 *   out_conv;  head.0, head.2, head.4 as [last_dim][32] (columns 4.. zero) with its bias padded to [32].
 * mi355gs_dpt_head_tap_offset: the byte offset inside the scratch at which the call leaves intermediate `which`, channels-last with
 *   F channels: 0..3 = L[0..3], 4..7 = path_4, path_3, path_2, path_1 (0 = refused; no buffer starts at offset 0).
 *
 * mi355gs_local_features: fc2(gelu(fc1(cat(hook0, hook3)))) per token, [dim_tokens[0] + dim_tokens[3] -> mlp_hidden ->
 *   (local_feat_dim + two_confs) 256], pixel_shuffle(16), desc [E][H][W][local_feat_dim] = the first local_feat_dim channels over
 *   their norm, desc_conf [E][H][W] = desc_conf_vmin + min(exp(last channel), desc_conf_vmax - desc_conf_vmin) when two_confs
 *   (else desc_conf is not written and may be NULL).  weights: fc1 [K][hidden] + bias, fc2 [hidden][out] + bias.
 *
 * scratch: the query's bytes of device memory, 16-byte aligned, owned by the caller (0 = the sizes are refused).  Launches on
 * the caller's stream; no allocation, no memset, no host synchronisation.
 * Limits (MI355GS_EINVAL beyond them, as for null pointers and weights, hooks, scratch or raw4 off a 16-byte boundary):
 * dim_tokens multiples of 32 in [32, 4096]; layer_dims multiples of 32 in [32, 1024]; feature_dim a multiple of 64 in [64, 256]
 * (F / 2 <= 128); last_dim a multiple of 32 in [32, 128]; mlp_hidden a multiple of 32 in [32, 32768]; local_feat_dim in [1, 255];
 * vmax > vmin; Ht Wt <= 4096; E <= 65535; 4 E H W <= 2^31 - 1 (callers split E).
 * ---------------------------------------------------------------------------------------------- */
typedef struct mi355gs_dpt_config {
  int dim_tokens[4];
  int layer_dims[4];
  int feature_dim, last_dim;
  int mlp_hidden, local_feat_dim, two_confs;
  float conf_vmin, conf_vmax;
  float desc_conf_vmin, desc_conf_vmax;
} mi355gs_dpt_config;
size_t mi355gs_dpt_head_scratch_bytes(const mi355gs_dpt_config* cfg, int Ht, int Wt, int E);
size_t mi355gs_dpt_head_tap_offset(const mi355gs_dpt_config* cfg, int Ht, int Wt, int E, int which);
int mi355gs_dpt_head(void* stream, const mi355gs_dpt_config* cfg, const float* weights, int Ht, int Wt, int E, const float* const hooks[4],
                     void* scratch, float* pts3d, float* conf, float* raw4);
size_t mi355gs_local_features_scratch_bytes(const mi355gs_dpt_config* cfg, int Ht, int Wt, int E);
int mi355gs_local_features(void* stream, const mi355gs_dpt_config* cfg, const float* weights, int Ht, int Wt, int E, const float* hook0,
                           const float* hook3, void* scratch, float* desc, float* desc_conf);

/* ----------------------------------------------------------------------------------------------
 * PNG files of 8-bit RGB frames, encoded on the device (csrc/png.hip).  frames: uint8 [N][H][W][3] in device memory, any base
 * address (a slice of a stack is fine).  out receives the N files back to back: file i is out[offsets[i] : offsets[i+1]], offsets
 * a device array of N + 1.  Every file is: signature, IHDR (8-bit RGB, no interlace), one IDAT per block of rows_per_block
 * filtered rows (0: the largest R with R (3 W + 1) <= 65536, at least 1; the last block holds the remaining rows), one IDAT with
 * the 4 Adler-32 bytes, IEND.  Every row is Paeth-filtered (filter byte 4).  A block is one dynamic-Huffman deflate block of
 * literals only (no LZ77 matches: what zlib's Z_HUFFMAN_ONLY produces) under an OPTIMAL code of at most 15 bits per symbol
 * (minimum sum of count x length over the block's 256 literals and the end-of-block symbol), followed by an empty stored block,
 * so that every block ends on a byte; the zlib header 78 01 opens the first block's chunk.  The price of leaving matches out is
 * a floor of one bit per byte: a constant-colour frame comes to 1/8 of its raw size.
 *   Size: a block of n filtered bytes gives at most (2 for a frame's first) + ceil((1106 + 9 (n + 1) + 3) / 8) + 4 data bytes;
 *   mi355gs_png_rgb8_stream_bytes is that bound over all N files with their framing, the size `out` must have.  The bytes of
 *   `out` behind offsets[N] are not written.
 * Three launches per call whatever N is, on the caller's stream; no host synchronisation, no allocation, no memset.  scratch: the
 * scratch-size query's bytes of device memory, 16-byte aligned, owned by the caller.  Both queries return 0 for sizes the call
 * refuses.  Limits (MI355GS_EINVAL beyond them, as for null pointers, non-positive sizes, a negative rows_per_block, a scratch
 * pointer that is not 16-byte aligned and an offsets pointer that is not 8-byte aligned): N <= 65535, W <= 21845,
 * rows_per_block (3 W + 1) <= 65536, N x ceil(H / rows_per_block) <= 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_png_rgb8_scratch_bytes(int N, int H, int W, int rows_per_block);
size_t mi355gs_png_rgb8_stream_bytes(int N, int H, int W, int rows_per_block);
int mi355gs_png_rgb8(void* stream, int N, int H, int W, int rows_per_block, const uint8_t* frames, void* scratch, uint8_t* out,
                     int64_t* offsets);

/* ----------------------------------------------------------------------------------------------
 * Baseline JPEG files of 8-bit RGB frames, encoded on the device (csrc/jpeg.hip): the frames of a Motion-JPEG video
 * (instantsplat_amd/video.py).  frames: uint8 [N][H][W][3] in device memory, any base address.  subsampling: 0 = 4:4:4, 2 = 4:2:0.
 * qtables: HOST array of 2 x 64 bytes, luma then chroma, natural (row-major) order, every entry 1..255; read during the call.
 * Every file is, in libjpeg's order: SOI, APP0 (JFIF 1.01, units 0, density 1 x 1), DQT 0 and DQT 1, SOF0 (components 1, 2, 3;
 * Y sampled 2 x 2 at 4:2:0; tables 0, 1, 1), DHT DC 0 / AC 0 / DC 1 / AC 1 (the typical tables of Annex K.3), DRI = the MCUs of
 * one MCU row, SOS, the entropy-coded data with RST0..RST7 in front of every MCU row but the first, EOI.  The arithmetic is
 * libjpeg's integer arithmetic throughout (16-bit fixed-point colour conversion, edge replication, h2v2 downsampling with the
 * alternating bias, the `islow` forward DCT, quantisation by truncating division of the rounded magnitude): the file equals,
 * byte for byte, what libjpeg / libjpeg-turbo write for the same tables with optimize off and one restart interval per MCU row.
 *   Capacity protocol: out receives the files back to back, file i at out[offsets[i] : offsets[i+1]].  offsets (device, N + 1) is
 *   ALWAYS exact, whatever out_bytes is.  File i is written — whole — exactly when offsets[i+1] <= out_bytes; no byte at or beyond
 *   out + out_bytes is ever written (out_bytes may be 0).  A caller may therefore pass a speculative buffer and encode the frames
 *   that did not fit again with the exact size.  mi355gs_jpeg_rgb8_stream_bytes is the worst case over all contents, framing
 *   included: per MCU row 2 x ceil(blocks x 1660 / 8) (1660 bits: a block's longest code; x 2: a zero behind every FF byte).
 * Three launches per call whatever N is (transform + count per MCU row; one scan; pack + store per MCU row), on the caller's
 * stream; no host synchronisation, no allocation, no memset.  scratch: the scratch-size query's bytes of device memory (the
 * quantised coefficients, 2 bytes each), 16-byte aligned, owned by the caller.  Both queries return 0 for sizes the call refuses.
 * Limits (MI355GS_EINVAL beyond them, as for null pointers, non-positive sizes, a subsampling other than 0 or 2, a table entry of
 * 0, a scratch pointer that is not 16-byte aligned and an offsets pointer that is not 8-byte aligned): H, W <= 65535 (the
 * format's), N <= 65535, 3 H W <= 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_jpeg_rgb8_scratch_bytes(int N, int H, int W, int subsampling);
size_t mi355gs_jpeg_rgb8_stream_bytes(int N, int H, int W, int subsampling);
int mi355gs_jpeg_rgb8(void* stream, int N, int H, int W, int subsampling, const uint8_t* qtables, const uint8_t* frames, void* scratch,
                      uint8_t* out, size_t out_bytes, int64_t* offsets);

/* ----------------------------------------------------------------------------------------------
 * The tail of the init stage (reference init_geo.py:61-129 behind `compute_global_alignment`; utils/sfm_utils.py:250-432):
 * confidence statistics, co-visibility masks and the ordered compaction of V aligned pointmaps.  All arrays are device memory,
 * contiguous: pointmaps float [V][H][W][3], depthmaps / confidences float [V][H][W], images float [V][H][W][3] in [0,1],
 * intrinsics float [V][3][3], w2c float [V][4][4] (row-major), overlap uint8 [V][H][W] (a torch.bool tensor's memory; 1 =
 * co-visible, redundant).  Every call enqueues on the caller's stream; no allocation, no memset, no host synchronisation, no
 * atomics (results are the same bits run to run).  Limits (MI355GS_EINVAL beyond them, as for null pointers and non-positive
 * sizes; the scratch-size queries then return 0): V <= 256, V H W <= 2^31 - 1.
 *
 *   pointmap_stats (2 launches): stats[v] = (min of depthmaps[v], max of depthmaps[v], sum of confidences[v]) as three doubles —
 *     min and max are the float32 values (a NaN propagates, as numpy's), the sum is accumulated in double in a fixed order.  The
 *     pass also CLEARS overlap: the masks need no memset.  scratch: mi355gs_pointmap_stats_scratch_bytes() bytes.
 *   covis_masks (1 launch over all V (V - 1) / 2 pairs; none for V == 1): `compute_co_vis_masks` (utils/sfm_utils.py:375-415).
 *     order: HOST array of V ints, a permutation of 0 .. V-1 (the confidence ranking, or 0 .. V-1).  For the view c of rank i and
 *     every point of the views of rank j < i: projection in double from the float32 inputs (cam = E [p,1], h = K cam, x = h0 / h2,
 *     y = h1 / h2), valid when 0 <= x < W and 0 <= y < H on the doubles, pixel = truncation; the point's depth in its own view,
 *     normalised in float32 with the min / max over all views ranked before c, against c's depth at the pixel normalised with c's
 *     own min / max; |difference| < depth_threshold (float32) stores 1 into overlap[c][y][x].  stats: what pointmap_stats wrote
 *     for these depthmaps; overlap: cleared by that call (or by the caller).  The first-ranked view is never marked.
 *   compact_pointmaps (3 launches: count per block of 1024 elements, a one-workgroup scan that loops over any number of block
 *     counts, ordered scatter): over the n = V H W elements in memory order, those with overlap == 0 (overlap null: all) go to
 *     out_points [M][3], out_rgb8 [M][3] ((uint8)(clamp(image, 0, 1) * 255.f): one float32 multiply, truncation — what
 *     `save_points3D` and storePly's uint8 fields make of the colours) and out_confidence [M][1], in the same order.  The out
 *     arrays must hold n rows.  M goes to *count_dev (device int32) and, when count_host is non-null, to that word too: host
 *     memory the device can write (pinned, mapped), read by the host once the stream has passed the call.
 *     scratch: mi355gs_compact_scratch_bytes(n) bytes.
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_pointmap_stats_scratch_bytes(int V, int H, int W);
int mi355gs_pointmap_stats(void* stream, int V, int H, int W, const float* depthmaps, const float* confidences, uint8_t* overlap,
                           void* scratch, double* stats);
int mi355gs_covis_masks(void* stream, int V, int H, int W, const int32_t* order, const float* pointmaps, const float* depthmaps,
                        const float* intrinsics, const float* w2c, const double* stats, float depth_threshold, uint8_t* overlap);
size_t mi355gs_compact_scratch_bytes(int64_t n);
int mi355gs_compact_pointmaps(void* stream, int64_t n, const uint8_t* overlap, const float* pointmaps, const float* images,
                              const float* confidences, void* scratch, float* out_points, uint8_t* out_rgb8, float* out_confidence,
                              int32_t* count_dev, int32_t* count_host);

/* ----------------------------------------------------------------------------------------------
 * The global alignment loop (reference dust3r/cloud_opt/base_opt.py:326-366 `global_alignment_loop` over
 * dust3r/cloud_opt/optimizer.py:188-201 `PointCloudOptimizer.forward`; run by init_geo.py:48 with 300 iterations and by
 * init_test_pose.py:59 with 500): V images of H x W, E directed edges (i, j) that cover every image, n = H W.  Per iteration a
 * log-depth map, a camera pose and a focal per image and a similarity transform per edge take one Adam step (betas 0.9 / 0.9,
 * eps 1e-8) on
 *   loss = (sum_e sum_p wi_e[p] |X_i[p] - M_e A_e[p]| + sum_e sum_p wj_e[p] |X_j[p] - M_e B_e[p]|) / (E n),   w = log(conf),
 *   X_v[p] = R_v (d u / f, d v / f, d) + T_v with d = exp(depth_log), (u, v) = (col, row) - pp, f = exp(focal_log / 20),
 *   pp = (W / 2, H / 2) + 10 pp_raw;  R = rotation of q / |q| (q scalar-last, x y z w), T = sign(t) expm1(|t|);
 *   M_e = sigma_e [R_e | T_e], sigma_e = exp(s_e) exp(log(base_scale) - mean(s)) with MI355GS_ALIGN_NORM_PW_SCALE, else exp(s_e).
 * The gradient of the norm at a zero residual is 0.  State, all device float, contiguous: depth_log [V][n], im_pose [V][7]
 * (q, t), focal_log [V], pp_raw [V][2] (constant), pw_pose [E][8] (q, t, s); the Adam moments m_* / v_* have the shapes of their
 * parameters.  Every call enqueues on the caller's stream.  A run makes 1 + 3 niter launches and nothing else: no allocation, no
 * memset, no event, no host synchronisation, no float atomics — two runs from the same state give the same bits.  (The handle's
 * FIRST call, whichever it is, also copies the edge-side tables to the device and waits for that copy.)
 *
 *   workspace_bytes / create / destroy: the handle pattern of the tracker.  edges: HOST array [E][2].  flags: MI355GS_ALIGN_*
 *     below, the reference's requires_grad switches and norm_pw_scale (optimizer.py:66-91).  create returns null, and
 *     workspace_bytes 0, for a null pointer, a non-positive size, an edge with i == j or an index outside [0, V), an image that
 *     no edge covers, V > 256, E > 65535, E H W > 2^31 - 1 (or H W > 2^31 - 1025), flags outside the mask, base_scale <= 0.
 *   pack: the handle's 16-byte records (x, y, z, log conf) from pred_i / pred_j [E][n][3] and conf_i / conf_j [E][n] (the
 *     reference's _stacked_pred_i / _j and conf_i / conf_j, optimizer.py:50-57); once per problem, before grad / run.
 *   grad: the loss and every gradient at the given state, nothing updated (tests; as mi355gs_trainer_grad).
 *   run: niter iterations (base_opt.py:349-366).  step_table: device float [niter][4], row k = (-lr_k / (1 - 0.9^t),
 *     sqrt(1 - 0.9^t), 0, 0) with t the optimizer's step count at iteration k and lr_k the schedule's rate (base_opt.py:352-357),
 *     formed on the host.  losses[k] = the loss of iteration k, before its step.  Groups whose flag is off keep their bits.
 *     niter == 0 does nothing.
 *   points: get_pts3d and get_depthmaps (optimizer.py:164-186): pts3d [V][n][3], depth [V][n].
 * ---------------------------------------------------------------------------------------------- */
#define MI355GS_ALIGN_OPT_DEPTH 1       /* im_depthmaps.requires_grad */
#define MI355GS_ALIGN_OPT_IM_POSES 2    /* im_poses.requires_grad: off after preset_pose (optimizer.py:66-81) */
#define MI355GS_ALIGN_OPT_FOCALS 4      /* im_focals.requires_grad: off after preset_focal (optimizer.py:83-91) */
#define MI355GS_ALIGN_OPT_PW_POSES 8    /* pw_poses.requires_grad */
#define MI355GS_ALIGN_NORM_PW_SCALE 16  /* base_opt.py:176-182 get_pw_norm_scale_factor */
size_t mi355gs_align_workspace_bytes(int V, int H, int W, int E, int flags);
void* mi355gs_align_create(void* workspace, int V, int H, int W, const int32_t* edges, int E, int flags, float base_scale);
void mi355gs_align_destroy(void* handle);
/* optimizer.py:50-57 */
int mi355gs_align_pack(void* handle, void* stream, const float* pred_i, const float* pred_j, const float* conf_i, const float* conf_j);
/* optimizer.py:188-201 and its autograd */
int mi355gs_align_grad(void* handle, void* stream, const float* depth_log, const float* im_pose, const float* focal_log, const float* pp_raw,
                       const float* pw_pose, float* g_depth_log, float* g_im_pose, float* g_focal_log, float* g_pw_pose, float* loss);
/* base_opt.py:326-366 */
int mi355gs_align_run(void* handle, void* stream, int niter, const float* step_table, float* depth_log, float* im_pose, float* focal_log,
                      const float* pp_raw, float* pw_pose, float* m_depth_log, float* v_depth_log, float* m_im_pose, float* v_im_pose,
                      float* m_focal_log, float* v_focal_log, float* m_pw_pose, float* v_pw_pose, float* losses);
/* optimizer.py:164-186 */
int mi355gs_align_points(void* handle, void* stream, const float* depth_log, const float* im_pose, const float* focal_log,
                         const float* pp_raw, const float* pw_pose, float* pts3d, float* depth);
/* the handle's records: device float [2 E][n][4], record (e, side) at index 2 e + side (side 0 = i), (x, y, z, log conf) */
const float* mi355gs_align_records(void* handle);

/* ----------------------------------------------------------------------------------------------
 * The aligner's initialisation (reference dust3r/cloud_opt/init_im_poses.py:66-221 `init_minimum_spanning_tree` /
 * `init_from_pts3d`, dust3r/post_process.py:36-53): the sums over the n = H W points of a pointmap.  The tree, the walk over it and
 * which record feeds which image are the host's (instantsplat_amd/global_align.py).  Stateless calls on the caller's stream, device
 * arrays, float, contiguous; no allocation, no memset, no float atomics, no host synchronisation; two calls give the same bits.
 *
 *   init_workspace_bytes(B, n): the scratch of any call below with B jobs (rows, images) of n points; 0 for B outside [1, 65535],
 *     n < 1, n > 2^31 - 1025 or B n > 2^31 - 1.  Every call answers MI355GS_EINVAL for such sizes and for a null pointer.
 *   A batch side is (base, idx, job_stride, pt_stride): job b reads base + (idx ? idx[b] : b) * job_stride floats, point p at
 *     pt_stride * p (3: a pointmap; 4: the handle's records).  idx: device int32 [B] or null.
 *   init_means: means[r] = mean(x[r][0 .. n)), rows of n floats (the confidence means behind commons.py:20-25).
 *   init_register: per job the weighted similarity registration tgt ~ s R src + T with roma's rigid_points_registration(...,
 *     compute_scaling = True) conventions: weighted centroids, M = sum w yh xh^T, R the special-orthogonal Procrustes solution
 *     (last singular direction flipped when det < 0), s = (sum of the signed singular values) / sum w |xh|^2, T = cy - s R cx.
 *     weights null: unit weights.  Two passes (centroids, then moments of the centred points), 4 launches.
 *     srt [B][16]: s, R row-major [9], T [3], 0 0 0.  pw_pose [B][8] or null: quaternion (x y z w) of R, signed_log1p(T / s), log s.
 *   init_apply: dst[p] = s R src[p] + T with (s, R, T) one srt row in device memory (null: a copy); dst [n][3].
 *   init_focals: per job the Weiszfeld focal of `estimate_focal_knowing_depth` (principal point (W / 2, H / 2), closed-form start,
 *     10 re-weightings, clipped at 0 from below): 22 launches for the whole batch.
 *   init_state (init_im_poses.py:115-129): factor = norm_pw_scale ? exp(log(base_scale) - mean(pw_pose[:, 7])) : 1; pts3d
 *     [V][n][3] *= factor in place; image v's pose is [R | factor T] of srt row pose_row[v] (< 0: identity); depth_log = log(z of
 *     inv(pose) pts3d) with NaN and -inf -> 0, +inf -> FLT_MAX; im_pose = (quaternion of R, signed_log1p(T)); focal_log =
 *     20 log(focal) with focal = focals[focal_row[v]] (focal_mode 0; focal_row < 0: 20 log(max(H, W))), the mean of those V values
 *     (1) or known_focal (2).  V <= 256, E <= 65535.
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_align_init_workspace_bytes(int B, int n);
int mi355gs_align_init_means(void* workspace, void* stream, int rows, int n, const float* x, float* means);
int mi355gs_align_init_register(void* workspace, void* stream, int B, int n, const float* src, const int32_t* src_idx, long long src_job_stride,
                                int src_pt_stride, const float* tgt, const int32_t* tgt_idx, long long tgt_job_stride, const float* weights,
                                const int32_t* w_idx, long long w_job_stride, float* srt, float* pw_pose);
int mi355gs_align_init_apply(void* stream, int n, const float* src, int src_pt_stride, const float* srt, float* dst);
int mi355gs_align_init_focals(void* workspace, void* stream, int B, int H, int W, const float* src, const int32_t* src_idx,
                              long long src_job_stride, int src_pt_stride, float* focals);
int mi355gs_align_init_state(void* workspace, void* stream, int V, int E, int H, int W, int norm_pw_scale, float base_scale, int focal_mode,
                             float known_focal, const float* srt, const int32_t* pose_row, const float* focals, const int32_t* focal_row,
                             const float* pw_pose, float* pts3d, float* depth_log, float* im_pose, float* focal_log);

/* ----------------------------------------------------------------------------------------------
 * Adaptive density control (reference scene/gaussian_model.py:328-477 and train.py:195-206): densification statistics, and one
 * clone / split / prune event as a plan (decisions, counts, scan) and an apply (one ordered scatter of every per-Gaussian row into
 * the caller's new buffers).  All arrays are device memory, contiguous; every call enqueues on the caller's stream; no allocation,
 * no memset, no host synchronisation, no atomics (results are the same bits run to run).  Limits (MI355GS_EINVAL beyond them, as
 * for null required pointers; the scratch-size query then returns 0): P >= 1, 1 <= N <= 8, P (N + 1) <= 2^31 - 1.
 *
 *   density_stats (1 launch): for every row with filter[i] != 0 (filter null: radii[i] > 0): grad_accum[i] += sqrt(gx gx + gy gy)
 *     of grad[i * grad_stride + 0 / 1] (torch's order: square, add, correctly rounded sqrt), denom[i] += 1 and, with radii and
 *     max_radii given, max_radii[i] = max(max_radii[i], radii[i]).
 *   density_plan (2 launches): flags say what the event does.
 *       CLONE   rows with |g| >= max_grad and max(exp(scaling)) <= dense_limit gain a copy (densify_and_clone)
 *       SPLIT   rows with g >= max_grad and max(exp(scaling)) > dense_limit are replaced by N children (densify_and_split)
 *       PRUNE   rows are removed: those of `mask` (uint8, non-zero = remove: prune_points), or with mask null those with
 *               sigmoid(opacity) < min_opacity and, with SCREEN, max_radii > max_screen_size or max(exp(scaling)) > world_limit
 *               (densify_and_prune:467-471).  The mask is evaluated for the row, for its clone and for its children, whose
 *               scaling is log(exp(scaling) / child_div), child_div = (float)(0.8 N).
 *     g is grads[i] (0 for i >= n_grads: the padded gradient) when grads is given, else grad_accum[i] / denom[i] with NaN -> 0.
 *     Whenever CLONE or SPLIT is set the screen-size term sees radii of 0 for every row, as in the reference, where
 *     densification_postfix clears max_radii2D before the mask is formed; with PRUNE alone it sees max_radii.  max_radii is read
 *     in that one form only (PRUNE | SCREEN, no mask, no CLONE / SPLIT), where null is MI355GS_EINVAL; elsewhere it may be null.
 *     code [P]: bit 0 the row survives, bit 1 it has a surviving clone, bit 2 it is split, bit 3 it was selected for cloning,
 *     bit 8 + k its child k survives.  scratch: mi355gs_density_scratch_bytes(P, N) bytes, read by density_apply.
 *     totals_host: null, or 16 int32 of host memory the device can write (pinned, mapped), valid once the stream has passed the
 *     call: [0] surviving originals, [1] surviving clones, [2] surviving children, [3] rows built and pruned again, [4] rows
 *     selected for splitting, [5] the new P, [6] rows selected for cloning, [8 + k] first output row of the children of copy k.
 *   density_apply (1 launch): out rows in the reference's order — surviving originals in index order, surviving clones in index
 *     order, surviving children of copy 0 in index order, copy 1, ... (`.repeat(N, 1)`: block-repeated).  in / out: host arrays of
 *     MI355GS_DENSITY_TENSORS device pointers indexed by the constants below; the six parameters are required (f_rest not when
 *     rest_width, its floats per row, is 0), the others move where both sides are given.  exp_avg / exp_avg_sq: survivors keep
 *     theirs, appended rows get zeros.  per_point_lr: a clone or child inherits its parent's.  The statistics are zeroed when
 *     CLONE or SPLIT is set and compacted otherwise.  A child's position is R(q) (exp(scaling) * z) + xyz with R the rotation of
 *     the normalised raw quaternion and z = noise[k n_selected + rank], rank counting the split rows in index order; noise:
 *     [noise_rows][3] unit normals, required with noise_rows >= N n_selected when n_selected (totals [4], as the host read it)
 *     is not 0.  out_rows: rows the out tensors hold (totals [5]); no row beyond it is written.  Every `in` pointer is 16-byte
 *     aligned, as is out's rotation.
 *   reset_opacity (1 launch): opacity = inverse_sigmoid(min(sigmoid(opacity), 0.01)) in place; exp_avg / exp_avg_sq (null or [P])
 *     are zeroed.
 * ---------------------------------------------------------------------------------------------- */
#define MI355GS_DENSITY_CLONE 1
#define MI355GS_DENSITY_SPLIT 2
#define MI355GS_DENSITY_PRUNE 4
#define MI355GS_DENSITY_SCREEN 8
#define MI355GS_DENSITY_XYZ 0
#define MI355GS_DENSITY_F_DC 1
#define MI355GS_DENSITY_F_REST 2
#define MI355GS_DENSITY_OPACITY 3
#define MI355GS_DENSITY_SCALING 4
#define MI355GS_DENSITY_ROTATION 5
#define MI355GS_DENSITY_EXP_AVG 6      /* + the parameter's index */
#define MI355GS_DENSITY_EXP_AVG_SQ 12  /* + the parameter's index */
#define MI355GS_DENSITY_PER_POINT_LR 18
#define MI355GS_DENSITY_GRAD_ACCUM 19
#define MI355GS_DENSITY_DENOM 20
#define MI355GS_DENSITY_MAX_RADII 21
#define MI355GS_DENSITY_TENSORS 22
int mi355gs_density_stats(void* stream, int P, const float* grad, int grad_stride, const uint8_t* filter, const int32_t* radii,
                          float* grad_accum, float* denom, float* max_radii);
size_t mi355gs_density_scratch_bytes(int P, int N);
int mi355gs_density_plan(void* stream, int P, int N, int flags, const float* grad_accum, const float* denom, const float* grads,
                         int64_t n_grads, const uint8_t* mask, const float* max_radii, const float* scaling, const float* opacity,
                         float max_grad, float dense_limit, float min_opacity, float max_screen_size, float world_limit,
                         float child_div, uint32_t* code, void* scratch, int32_t* totals_host);
int mi355gs_density_apply(void* stream, int P, int N, int flags, int rest_width, const uint32_t* code, const void* scratch,
                          const float* noise, int64_t noise_rows, int64_t n_selected, float child_div, const void* const* in,
                          void* const* out, int64_t out_rows);
int mi355gs_reset_opacity(void* stream, int P, float* opacity, float* exp_avg, float* exp_avg_sq);

/* ----------------------------------------------------------------------------------------------
 * Resizing 8-bit RGB images on the device (csrc/resample.hip): PIL's `Image.resize` for 8-bit images, byte for byte, with the
 * crop and the conversion to float that follow it in the reference's loaders (utils/general_utils.py:21-27 PILtoTorch;
 * dust3r/utils/image.py:63-70,73-126 load_images).  images: uint8 [N][H][W][3] in device memory, any base address; the call
 * resizes each to Hout x Wout and produces the window x0 <= x < x0 + w, y0 <= y < y0 + h of the result.
 *   Tables (device memory, built by the caller as PIL's precompute_coeffs + normalize_coeffs_8bpc build them:
 *   instantsplat_amd/resample.py `resample_coeffs`): kx int32 [Wout][ksize_x], coefficients with 22 fractional bits, and bx int32
 *   [Wout][2] = (first source column, number of taps) per output column; ky [Hout][ksize_y] and by [Hout][2] likewise for rows.
 *   kx NULL: the horizontal pass is skipped, Wout must equal W; ky NULL: the vertical pass is skipped, Hout must equal H.
 *   Arithmetic, per pass and channel: acc = 2^21 + sum over the taps of k[t] * byte[first + t] in 32-bit integers, result =
 *   clip(acc >> 22, 0, 255); a coefficient enters as its low 24 bits, signed (PIL's stay below 2^23 in magnitude), and the sum wraps.
 *   The horizontal pass runs first and stores 8 bits, as PIL's does.  Taps that a table places outside
 *   the image (or outside its row of the table) are not read, whatever the tables hold.
 *   Outputs, each NULL or device memory, one of them at least, all written by the last pass that runs:
 *     rgb8 uint8 [N][h][w][3]; unit float [N][3][h][w] = (float)v / 255.0f; normalized float [N][3][h][w] =
 *     ((float)v / 255.0f - 0.5f) / 0.5f, every operation in IEEE float32, rounded once.
 *   row0, rows, scratch: read only when both passes run.  The horizontal pass then produces the source rows row0 .. row0+rows-1
 *   for the window's columns into scratch (mi355gs_resample_rgb8_scratch_bytes(N, rows, w) bytes of device memory, owned by the
 *   caller): the rows the window's vertical taps reach, i.e. by[y0][0] .. by[y0+h-1][0] + by[y0+h-1][1] - 1.
 * Launches: one per pass that runs; one copy / convert launch when both are skipped.  On the caller's stream; no host
 * synchronisation, no allocation, no memset, no atomics.  Limits (MI355GS_EINVAL beyond them, as for null images, no output, a
 * window outside the result, a missing bounds table or ksize <= 0 beside a table, a size change without its table, a null
 * scratch or a row range outside the source when both passes run; the scratch query then returns 0): N and every size
 * <= 65535, 3 H W and 3 Hout Wout <= 2^31 - 1.
 * ---------------------------------------------------------------------------------------------- */
size_t mi355gs_resample_rgb8_scratch_bytes(int N, int rows, int w);
int mi355gs_resample_rgb8(void* stream, int N, int H, int W, int Hout, int Wout, const uint8_t* images, const int32_t* kx,
                          const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, int x0, int y0, int w,
                          int h, int row0, int rows, void* scratch, uint8_t* rgb8, float* unit, float* normalized);

#ifdef __cplusplus
}
#endif
#endif /* MI355GS_H */
