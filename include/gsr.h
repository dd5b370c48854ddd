/*
 * gsr.h -- C-ABI of the MI355X-native Gaussian-splatting rasterizer (libgsr_hip.so).
 *
 * This is the drop-in boundary of the hot path: plain pointers and sizes, no torch
 * types.  Every entry point replaces one L0 interface of the reference
 * (HuajianUP/Photo-SLAM); the LibTorch wrappers RasterizeGaussiansCUDA /
 * RasterizeGaussiansBackwardCUDA / markVisible / distCUDA2 sit directly on top
 * (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * All pointers are DEVICE pointers (gfx950 HBM) unless stated; fp32 throughout.
 * A null pointer stands for an absent optional exactly as in the reference, where
 * an empty tensor yields data_ptr()==nullptr (src/gaussian_rasterizer.cpp:209-219,
 * cuda_rasterizer/forward.cu:205,241).
 * The library owns no device memory: scratch comes from the caller through
 * gsr_alloc_fn (the reference's std::function<char*(size_t)> resize callbacks,
 * cuda_rasterizer/rasterizer.h:36-38, src/rasterize_points.cu:28-34).
 * All work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null
 * stream).  Functions return GSR_OK or a negative gsr_status; they never throw.
 */
#ifndef GSR_H
#define GSR_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum gsr_status {
	GSR_OK = 0,
	GSR_ERR_INVALID_ARG = -1,   /* bad shape / forbidden null / inconsistent optional combination */
	GSR_ERR_ALLOC = -2,         /* a gsr_alloc_fn returned NULL */
	GSR_ERR_HIP = -3,           /* a HIP runtime call or kernel launch failed (see gsr_last_hip_error) */
	GSR_ERR_UNSUPPORTED = -4    /* e.g. tile grid larger than 65535 in one dimension */
} gsr_status;

/* Resize-and-return-pointer callback; must return a device pointer to at least
 * `bytes` bytes, 16-byte aligned (torch allocations are 512-byte aligned).
 * Replaces std::function<char*(size_t)> of Rasterizer::forward
 * (cuda_rasterizer/rasterizer.h:36-38). */
typedef char* (*gsr_alloc_fn)(void* ctx, size_t bytes);

/* Extension of the extension below: LAZY Adam steps for the SH rows of culled Gaussians (NULL in gsr_sh_adam = every row takes
 * every step when it happens).  A Gaussian the view culls gets a zero SH gradient, and a zero-gradient Adam step of a row --
 * m <- b1 m, v <- b2 v, p <- p - step_size m / (sqrt(v) / sqrt(1 - b2^t) + eps) -- depends on nothing but the row and the
 * step's scalars.  With row_step set the library takes such steps LATER, several at a time with the row in registers: the
 * same arithmetic in the same order (results bit-identical to the eager update, tests/test_lazy_sh_adam.py), one HBM round
 * trip of the row's 1152 bytes instead of one per step.  row_step[i] = number of Adam steps row i has taken.  A row is
 * brought up to date
 *   - by gsr_forward when it becomes visible, BEFORE its coefficients are evaluated (pass the same gsr_sh_adam to
 *     gsr_forward_args.sh_adam and gsr_backward_args.sh_adam of a step);
 *   - by gsr_backward for a rotating 1/window of the row blocks per step, so that no row ever lags by more than `window`
 *     steps (the past learning rates the caller has to remember);
 *   - by gsr_sh_adam_flush for all rows: REQUIRED before anything else reads or writes the tensor or its moments (densify /
 *     prune, save, a dense optimizer step, another exchange mode).
 * Contract: when the first lazy step `step` is taken every row_step[i] == step - 1; from then on every step's forward and
 * backward get the struct with the same `window` until a flush. */
#define GSR_SH_LAZY_WINDOW 32
typedef struct gsr_sh_adam_lazy {
	int* row_step;                          /* [P] device ints, read and written */
	int window;                             /* 2 .. GSR_SH_LAZY_WINDOW */
	double lr_past[GSR_SH_LAZY_WINDOW];     /* [k-1] = lr of Adam step (step - k), k = 1 .. window-1 (entries of steps < 1 unused) */
	double lr_tail_past[GSR_SH_LAZY_WINDOW];
} gsr_sh_adam_lazy;

/* Extension: Adam state of the [P,16,3] SH tensor for the fused update inside gsr_backward (see
 * gsr_backward_args.sh_adam).  torch::optim::Adam semantics as gsr_adam_step; the first 3 floats of a row
 * (features_dc) use lr, the other 45 (features_rest) lr_tail. */
typedef struct gsr_sh_adam {
	float* param;                /* [P,16,3]: the SH tensor itself, UPDATED IN PLACE; gsr_backward requires param == shs (the
	                                const input pointer of the reference's parameter list stays const: the write goes
	                                through this one) */
	float* exp_avg;              /* [P,16,3] */
	float* exp_avg_sq;           /* [P,16,3] */
	double lr, lr_tail, beta1, beta2, eps;   /* double like torch::optim::AdamOptions: the bias corrections 1 - beta^step are
	                                            formed in double as torch does (0.999f instead of 0.999 is 1e-5 of the step) */
	int step;                    /* >= 1: the step being taken (bias correction) */
	const gsr_sh_adam_lazy* lazy; /* NULL = eager: every row takes the step in gsr_backward */
	/* Where the optimizer work that gsr_forward / gsr_backward fork next to their own kernels runs.  Zero in every field = the
	 * measured-best arrangement on MI355X (DESIGN.md sections 5, 9.1) -- a zero-initialised struct is the fast one.  None of
	 * them changes a result.  The environment variables named here OVERRIDE the fields when set (A/B handles of the bench
	 * sessions); a process that never sets them is governed by the fields alone. */
	int no_side_stream;          /* 1: no second stream at all -- the lazy rows' slice and the culled rows of the eager step run on
	                                the caller's stream (GSR_SH_ADAM_SIDE_STREAM=0 / 1) */
	int lazy_slice_late;         /* 1: this step's slice of the lazy rows is forked behind the backward blend instead of next to it
	                                (GSR_LAZY_SLICE_EARLY=0 / 1; measured: next to the blend C3 1.625 -> 1.613 ms) */
	int side_blocks;             /* eager mode: workgroups of the culled rows' kernel on the second stream; 0 = 256 (measured best
	                                of 64 / 256 / 1024 / 2048; GSR_SH_ADAM_SIDE_BLOCKS) */
} gsr_sh_adam;

/* Extension: optimizer-in-backward for the four per-Gaussian geometry tensors (see gsr_backward_args.geom_adam).  One entry per
 * tensor: torch::optim::Adam semantics as gsr_adam_step, each tensor with its own learning rate and step counter. */
typedef struct gsr_adam_tensor {
	float* param;                /* UPDATED IN PLACE */
	float* exp_avg;
	float* exp_avg_sq;
	double lr;
	int step;                    /* >= 1: the step being taken */
} gsr_adam_tensor;
typedef struct gsr_geom_adam {
	gsr_adam_tensor xyz;         /* [P,3]; param must be means3D */
	gsr_adam_tensor opacity;     /* [P]   the raw opacity (logits) */
	gsr_adam_tensor scaling;     /* [P,3]; param must be scales (log-scales) */
	gsr_adam_tensor rotation;    /* [P,4]; param must be rotations (unnormalised quaternions) */
	double beta1, beta2, eps;
} gsr_geom_adam;

/* Extension: opacity, scale and isotropy regularisers on the Gaussians a view sees (see gsr_backward_args.geom_reg).  With V the
 * Gaussians with radii > 0 in this view, o_i the activated opacity (the input, or its sigmoid under GSR_RAW_OPACITY; never the value
 * GSR_ANTIALIAS compensates), s_ik the activated scale (the input, or its exp under GSR_RAW_SCALING; WITHOUT scale_modifier),
 * m_i = (s_i0 + s_i1 + s_i2) / 3 and d_ik = s_ik - m_i:
 *   loss[0] = w_opacity   * sum_{i in V} o_i                      (the opacity L1 of 3DGS-MCMC)
 *   loss[1] = w_scale     * sum_{i in V} sum_k s_ik               (the scale L1 of 3DGS-MCMC)
 *   loss[2] = w_isotropic * sum_{i in V} sum_k |d_ik|             (the isotropic loss of MonoGS)
 *   dL/do_i  += w_opacity                                                   (* o (1 - o) under GSR_RAW_OPACITY)
 *   dL/ds_ik += w_scale + w_isotropic * (sgn d_ik - (1/3) sum_j sgn d_ij)   (* s_ik under GSR_RAW_SCALING), sgn 0 = 0
 * The terms join the opacity and scale gradients of the pass before those are written (dL_dopacity, dL_dscale) or consumed by the
 * fused geom_adam step; culled rows get nothing and no other output of the pass changes.  Three equal scales give d = 0 exactly
 * (d_ik is formed from the differences of the scales).  The weights are per Gaussian: a caller that wants MonoGS's mean over the
 * visible Gaussians divides by gsr_last_visible_count() (and by 3 for the two scale terms), as both hosts do.
 * loss: all three floats are written by every call that sets it (0 for P == 0 or a view that sees nothing), formed without atomics
 * -- one entry per workgroup and sum in `scratch`, added in double in a fixed order by one small extra launch -- so the same inputs
 * give the same bits on every run and in both GSR_BINNING_* arrangements.  loss == NULL: no entries, no extra launch, no scratch.
 * A struct whose three weights are 0 and whose loss is NULL behaves as NULL.
 * GSR_ERR_INVALID_ARG: a negative or non-finite weight; loss without scratch (or scratch not 4-byte aligned); w_scale or
 * w_isotropic non-zero with cov3D_precomp (no scales to regularise).  GSR_ERR_UNSUPPORTED: together with dL_dcolor_view /
 * packed_view (the multi-GPU exchange) or with the pose outputs.
 * Works with GSR_RAW_* in any combination (without a raw bit the gradient is that of the activated input, like every gradient of
 * this API), GSR_ANTIALIAS, dL_ddepth / dL_dalpha, sh_adam (eager and lazy), geom_adam, stat_*, colors_precomp and compact
 * [P,M,3] SH. */
typedef struct gsr_geom_reg {
	float w_opacity, w_scale, w_isotropic;  /* finite, >= 0; weights per Gaussian, already normalised by the caller */
	float* loss;                            /* [3] device floats or NULL: the three loss values of this view */
	char* scratch;                          /* gsr_geom_reg_scratch_bytes(P) device bytes; required iff loss != NULL */
} gsr_geom_reg;

/* Rasterizer::forward parameter list, cuda_rasterizer/rasterizer.h:35-59, 1:1. */
typedef struct gsr_forward_args {
	int P, D, M;                 /* #Gaussians, active SH degree, SH coeffs per channel stored */
	const float* background;     /* [3] */
	int width, height;
	const float* means3D;        /* [P,3] */
	const float* shs;            /* [P,M,3] or NULL */
	const float* colors_precomp; /* [P,3] or NULL (exactly one of shs / colors_precomp) */
	const float* opacities;      /* [P] */
	const float* scales;         /* [P,3] or NULL */
	float scale_modifier;
	const float* rotations;      /* [P,4] (r,x,y,z), NOT normalised in-kernel (forward.cu:127) */
	const float* cov3D_precomp;  /* [P,6] or NULL (exactly one of scales+rotations / cov3D_precomp) */
	const float* viewmatrix;     /* [16] = W2C^T row-major, i.e. element (r,c) at [4c+r].  The backward pass can differentiate with
	                                respect to viewmatrix, projmatrix and cam_pos: gsr_backward_args.dL_dviewmatrix and below */
	const float* projmatrix;     /* [16] = (Proj W2C)^T */
	const float* cam_pos;        /* [3] */
	float tan_fovx, tan_fovy;
	int prefiltered;
	float* out_color;            /* [3,H,W] written for every pixel */
	int* radii;                  /* [P] or NULL */
	/* Extension (0 = the reference contract: activated inputs).  Bit mask of GSR_RAW_*: the corresponding input
	 * holds the model's RAW parameter and the activation of GaussianModel (src/gaussian_model.cpp:48-62) is applied
	 * in-kernel: sigmoid(opacity), exp(scaling), normalize(rotation).  Saves the ~13 elementwise ATen launches
	 * (forward + autograd) GaussianRenderer::render otherwise spends per step. */
	int raw_params;
	/* Extension (NULL = the reference contract; consulted only when sh_adam->lazy is set, see gsr_sh_adam_lazy): the SH
	 * rows of visible Gaussians that lag behind (sh_adam->step - 1) take their missed zero-gradient Adam steps before their
	 * coefficients are evaluated -- the forward pass then WRITES sh_adam->param (== shs), the moments and row_step. */
	const gsr_sh_adam* sh_adam;
	/* Extension (NULL = the reference contract): a depth map and an alpha map, [H,W] each, written for every pixel; either may
	 * be set without the other.  For pixel p, with the same list entries, alpha_j, T_j and early stop as the colour blend:
	 *   out_depth[p] = sum_j z_j alpha_j T_j,   z_j = the view-space z of Gaussian j's mean, transformPoint4x3(mean, view).z
	 *                  (the value the depth sort keys on).  Not normalised and without a background term: an empty pixel has
	 *                  depth 0; the expected depth is out_depth / out_alpha.
	 *   out_alpha[p] = 1 - T_final[p], the T the forward pass keeps for the backward pass.
	 * Works with and without GSR_FORWARD_ONLY, in both GSR_BINNING_* arrangements, with GSR_CULL_EMPTY_TILES, colors_precomp,
	 * cov3D_precomp and GSR_RAW_*; out_color, radii and *num_rendered are the same, bit for bit, as without them.  P == 0 leaves
	 * them untouched, as out_color.  Gradients: gsr_backward_args.dL_ddepth / dL_dalpha. */
	float* out_depth;
	float* out_alpha;
	/* Extension (all NULL / 0 = the reference contract; read only with GSR_CONTRIBUTION in raw_params, see there): per-Gaussian
	 * contribution statistics of this render. */
	const float* pixel_weight;   /* [H,W] or NULL = all ones: w(p), every value finite and >= 0 */
	float* out_weight_sum;       /* [P] or NULL */
	float* out_weight_max;       /* [P] or NULL */
	int* out_n_touched;          /* [P] or NULL */
	int contribution_accumulate; /* 0: every element of the outputs is written.  1: sum += new (one float add), max = max(max, new),
	                                n_touched += new: a scoring pass over K keyframes is K renders with nothing in between */
	/* Extension (read only with GSR_FILTER_3D in raw_params, see there; without the bit the pointer is not read): the 3-D smoothing
	 * filter of every Gaussian, e.g. from gsr_filter3d_compute.  An input without a gradient. */
	const float* filter_3D;      /* [P] */
} gsr_forward_args;

#define GSR_RAW_OPACITY 1   /* opacities are logits */
#define GSR_RAW_SCALING 2   /* scales are log-scales */
#define GSR_RAW_ROTATION 4  /* rotations are unnormalised quaternions (normalised with eps 1e-12 like F::normalize) */
/* One more bit of gsr_forward_args.raw_params (ignored by gsr_backward), not about the inputs: the reference lists a Gaussian in
 * EVERY tile of the bounding square of its 3-sigma radius (duplicateWithKeys, rasterizer_impl.cu:70-111); most of those
 * instances blend into no pixel (alpha < 1/255 over the whole tile: 78 % of them at 2 M Gaussians @ 1080p).  With this bit the
 * instances of such tiles -- decided by the same conservative bound the blend kernels apply per 8x8 quad, on the tile's 16x16
 * rectangle -- are dropped in front of the tile sort.  The image and every gradient are the SAME, bit for bit (the dropped
 * pairs are pairs the reference `continue`s over at every pixel); what changes is internal: the sorted instance list is
 * shorter (num_rendered still counts the rectangles: it sizes the buffers), and n_contrib counts positions of the shorter
 * list.  0 = the reference's lists, bit for bit.  Measured: 26-40 % of the instances go, the sort and
 * the blend kernels gain what the test costs in the emission -- both hosts leave it off unless GSR_CULL_EMPTY_TILES=1. */
#define GSR_CULL_EMPTY_TILES 8
/* ... and one for introspection (ignored by gsr_backward): the forward pass ALSO leaves the 3-D covariances it computed in the
 * geometry buffer (24 bytes per visible Gaussian; the reference's geomState.cov3D).  Nothing in the library reads them back --
 * gsr_backward recomputes them from scales / rotations, the same arithmetic and the same bits -- so by default they are not
 * written; the test-suite's view into the buffer (tests/dev) asks for them. */
#define GSR_STORE_COV3D 16
/* ... and two that choose how the per-tile lists are built (ignored by gsr_backward; neither = the library decides by the size
 * of the view; the lists, the image and the gradients are the same either way, bit for bit).  DEPTH_FIRST: the Gaussians are
 * sorted by depth once (nine launches whatever the size), their instances emitted in that order, and the stable tile sort carries
 * the order into the tiles -- the least work per instance, the arrangement for large views.  TILE_FIRST: the visible Gaussians are
 * only compacted (ascending id) and every tile's list is sorted by depth on its own behind the tile sort, one workgroup per tile
 * in LDS -- eight launches fewer, the arrangement for the small and mid-size views a SLAM session starts with. */
#define GSR_BINNING_DEPTH_FIRST 32
#define GSR_BINNING_TILE_FIRST 64
/* ... and one for renders that no backward pass follows (a viewer, an evaluation pass, any no-grad render; ignored by
 * gsr_backward): out_color, radii and *num_rendered are the same, bit for bit, as without it, but nothing the backward pass
 * would need is prepared -- the binning buffer holds only the instance lists, their sort tables and one spare word per
 * instance (no gradient slots, no slot flags, no per-quad contribution flags), the image buffer only the tile ranges (no final
 * T, no last contributor), the forward blend stores neither, the clamp mask and the list of long runs are not written.
 * gsr_binning_bytes_for / gsr_image_bytes_for give the sizes it requests.  The three scratch buffers are NOT valid input to
 * gsr_backward: a cheap guard catches the usual mistake -- gsr_forward remembers, per thread, the geometry buffer of its last
 * forward-only call (a training forward on that buffer clears the record) and gsr_backward refuses that buffer with
 * GSR_ERR_INVALID_ARG.  A backward pass on another thread is not caught.
 * Works with both GSR_BINNING_* arrangements, GSR_CULL_EMPTY_TILES, colors_precomp, cov3D_precomp and GSR_RAW_*.
 * With sh_adam->lazy set (and only then: a non-lazy sh_adam is GSR_ERR_INVALID_ARG) the lazy rows are READ-ONLY: a visible row
 * that lags behind (sh_adam->step - 1) is evaluated at its caught-up value -- the same zero-gradient steps, the same arithmetic
 * as the training forward, taken in registers and LDS -- and nothing is written (not param, not the moments, not row_step).  A
 * caller whose tensor has taken S steps passes step = S + 1 and lr_past[0] = the learning rates of step S: the image is then
 * the one a training forward renders after gsr_sh_adam_flush. */
#define GSR_FORWARD_ONLY 128
/* ... and one that changes what is rendered (read by gsr_forward AND gsr_backward: it must be the same in both calls, like the
 * GSR_RAW_* bits; gsr_backward refuses, with GSR_ERR_INVALID_ARG, the geometry buffer of the calling thread's last training forward
 * when the bit differs).  ANTI-ALIASED rendering: the reference adds 0.3 to the diagonal of every projected 2-D covariance
 * (computeCov2D, forward.cu:74-113) and leaves the opacity alone, so a Gaussian smaller than a pixel deposits
 * sqrt(det(Sigma + 0.3 I) / det Sigma) times the alpha it should -- a factor that depends on the resolution of the render.  With
 * this bit the opacity is compensated (the 2-D filter normalisation of Mip-Splatting; `antialiasing` of upstream
 * diff-gaussian-rasterization, rasterize_mode="antialiased" of gsplat).  With Sigma = (a b; b c) the projected covariance BEFORE
 * the low-pass:
 *   h = sqrt(max(0.000025, det Sigma / det(Sigma + 0.3 I)))      the opacity every later stage uses = opacity_activated * h
 * in float32, every operation rounded on its own (no contraction), in this order:
 *   a1 = a + 0.3f;  c1 = c + 0.3f;  det1 = a1 * c1 - b * b      (the determinant the conic is formed from)
 *   det0 = a * c - b * b;  h2 = fmaxf(0.000025f, det0 / det1);  h = sqrtf(h2);  opacity = opacity_activated * h
 * (a, b, c in the operation order of computeCov2D; opacity_activated = the input, or its sigmoid under GSR_RAW_OPACITY).
 * Unchanged by the bit: the conic, the 3-sigma radius, the tile rectangle, radii, the sort keys, the lists and *num_rendered --
 * all those of Sigma + 0.3 I, bit for bit; only the opacity of the blend record differs, and the blend kernels, the bound of
 * GSR_CULL_EMPTY_TILES and out_depth / out_alpha all read that value.
 * gsr_backward: dL_dopacity = (the blend's gradient of the compensated opacity) * h, times o (1 - o) under GSR_RAW_OPACITY; and
 * dL/dh = that gradient * opacity_activated is chained through h(a, b, c) into the gradient of the 2-D covariance (zero where
 * the clamp 0.000025 is active), from where it reaches dL_dcov3D, the covariance part of dL_dmean3D, dL_dscale / dL_drot, the fused
 * geom_adam steps and the J^T dL/dT term of dL_dviewmatrix like every other covariance gradient.
 * Works with both GSR_BINNING_* arrangements, GSR_CULL_EMPTY_TILES, GSR_FORWARD_ONLY, GSR_RAW_*, colors_precomp, cov3D_precomp,
 * the depth / alpha maps and their gradients, the pose gradients, geom_adam, sh_adam and the view-factored exchange.  0 = the
 * reference's render, bit for bit, by the same kernels as before (the bit selects instantiations of its own). */
#define GSR_ANTIALIAS 256
/* ... and one that makes gsr_forward report what every Gaussian put into the image (ignored by gsr_backward).  radii > 0 says a
 * Gaussian is inside the frustum with a non-empty footprint, not that any pixel blends it.  For Gaussian g take every pixel p that
 * blends g in the colour blend -- the same list entries, the same power > 0 and alpha < 1/255 skips, the same T (1 - alpha) < 1e-4
 * stop as out_color -- with alpha_g(p) the blended alpha (at most 0.99), T_g(p) the transmittance in front of g, and w(p) =
 * gsr_forward_args.pixel_weight (NULL = 1):
 *   out_weight_sum[g] = sum_p w(p) alpha_g(p) T_g(p)
 *   out_weight_max[g] = max_p w(p) alpha_g(p) T_g(p), 0 if there is no such pixel
 *   out_n_touched[g]  = the number of such pixels with w(p) != 0
 * A Gaussian with radii == 0 gets 0 / 0 / 0.  Any subset of the three outputs may be NULL, but with the bit at least one is set;
 * the bit without an output, or an output (or pixel_weight) without the bit, is GSR_ERR_INVALID_ARG.  contribution_accumulate:
 * see the field.  The outputs are deterministic: the same inputs give the same bits on every run and in both GSR_BINNING_*
 * arrangements (no atomics: per-(tile quad, instance) partial results in the binning buffer, summed per Gaussian in a fixed
 * order); under GSR_CULL_EMPTY_TILES too.  sum_g out_weight_sum[g] = sum_p out_alpha[p] up to rounding when w = 1.
 * Works with and without GSR_FORWARD_ONLY, in both GSR_BINNING_* arrangements, with GSR_CULL_EMPTY_TILES, GSR_ANTIALIAS,
 * GSR_RAW_*, colors_precomp, cov3D_precomp, out_depth / out_alpha and the lazy sh_adam (read-only under GSR_FORWARD_ONLY);
 * out_color, radii, *num_rendered and the depth / alpha maps are the same, bit for bit, as without the bit, and gsr_backward on
 * the buffers of a training-form call gives the gradients it gives after a plain forward.  The binning buffer grows by 48 bytes
 * per instance: gsr_binning_bytes_for(R, raw_params) is the size requested.  P == 0 leaves the outputs untouched. */
#define GSR_CONTRIBUTION 512
/* ... and one that changes what is rendered (read by gsr_forward AND gsr_backward: the same value in both calls, exactly as
 * GSR_ANTIALIAS, and refused by gsr_backward in the same way when it differs from the forward call's).  The 3-D SMOOTHING FILTER of
 * Mip-Splatting, the other half of GSR_ANTIALIAS: every Gaussian is bounded from below by the sampling interval of the keyframes
 * that observe it, so that no view closer than any keyframe erodes it.  filter_3D[i] = f is a per-Gaussian INPUT (gsr_forward_args /
 * gsr_backward_args.filter_3D; gsr_filter3d_compute derives it from the keyframes) and has no gradient.  With s_k the activated scale
 * (the input, or its exp under GSR_RAW_SCALING; WITHOUT scale_modifier) and o the activated opacity (the input, or its sigmoid under
 * GSR_RAW_OPACITY), in float32, every operation rounded on its own, in this order:
 *   F   = f * f
 *   a_k = s_k * s_k + F          s'_k = sqrtf(a_k)          r_k = s_k / s'_k        (k = 0, 1, 2)
 *   c   = (r_0 * r_1) * r_2      o'   = o * c
 * Everything downstream sees (s', o') in place of (s, o): the covariance, scale_modifier, the radius, the h of GSR_ANTIALIAS (the
 * record holds (o c) h), the blend record's opacity, the bound of GSR_CULL_EMPTY_TILES, the depth and alpha maps, the contribution
 * statistics.  c = sqrt(det Sigma / det(Sigma + F I)) of Mip-Splatting, written as a product of ratios so that nothing underflows
 * for tiny scales; f = 0 gives s' = s and c = 1 exactly (scales whose squares do not underflow).  Division and square root are the
 * correctly rounded ones (the HIP compiler's default for float): gsr_forward and gsr_backward evaluate the same bits.
 * gsr_backward, with g_s' the gradient of the filtered scale and g_o' that of the filtered opacity (what the pass forms without
 * the bit):
 *   dL/ds_k = g_s'_k * r_k + g_o' * o * (r_{k+1} * r_{k+2}) * F / (a_k * s'_k)       dL/do = g_o' * c
 * then the raw chain rules as ever (* s_k under GSR_RAW_SCALING, * o (1 - o) under GSR_RAW_OPACITY).  o is recovered from the
 * record as o' / c, as under GSR_ANTIALIAS (the backward pass is given no opacities); a Gaussian with c == 0 (a scale that is
 * exactly 0 under a non-zero filter) renders nothing and gets no opacity term.  The gsr_geom_reg terms join AFTER this chain rule
 * and stay defined on the unfiltered s and o; stat_*, dL_dmean2D_abs and the pose gradients are unaffected except through the
 * changed render; dL_dcov3D is the gradient of the filtered covariance.
 * GSR_ERR_INVALID_ARG: the bit with filter_3D == NULL; the bit together with cov3D_precomp (no scales to filter).  A negative or
 * non-finite entry is the caller's error and is not checked on the device.  GSR_ERR_UNSUPPORTED: together with dL_dcolor_view /
 * packed_view (the multi-GPU exchange).
 * Works with geom_adam (the fused step consumes the filtered chain rule's gradients), sh_adam (eager and lazy), dL_ddepth /
 * dL_dalpha, GSR_ANTIALIAS, GSR_FORWARD_ONLY, GSR_CONTRIBUTION, GSR_CULL_EMPTY_TILES, both GSR_BINNING_* arrangements, geom_reg,
 * dL_dmean2D_abs and the pose outputs.  0 = the render and the gradients without it, bit for bit, by the same kernels as before
 * (the bit selects instantiations of its own). */
#define GSR_FILTER_3D 1024

/* Rasterizer::forward, cuda_rasterizer/rasterizer_impl.cu:198-336.
 * Fills out_color and radii, returns the number of (tile, Gaussian) instances in
 * *num_rendered.  The three scratch buffers are opaque and must be handed unchanged
 * to gsr_backward.  One host synchronisation (to size the binning buffer), as the
 * reference (rasterizer_impl.cu:281).  P == 0 is a valid no-op that leaves
 * out_color untouched (src/rasterize_points.cu:81). */
int gsr_forward(const gsr_forward_args* args,
                gsr_alloc_fn geometryBuffer, void* geometry_ctx,
                gsr_alloc_fn binningBuffer, void* binning_ctx,
                gsr_alloc_fn imageBuffer, void* image_ctx,
                void* stream, int* num_rendered);


/* Rasterizer::backward parameter list, cuda_rasterizer/rasterizer.h:61-91. */
typedef struct gsr_backward_args {
	int P, D, M, R;
	const float* background;
	int width, height;
	const float* means3D;
	const float* shs;
	const float* colors_precomp;
	const float* scales;
	float scale_modifier;
	const float* rotations;
	const float* cov3D_precomp;
	const float* viewmatrix;     /* these three have gradients: dL_dviewmatrix / dL_dprojmatrix / dL_dcampos below */
	const float* projmatrix;
	const float* campos;
	float tan_fovx, tan_fovy;
	const int* radii;            /* [P] or NULL (then the copy inside geom_buffer is used) */
	char* geom_buffer;
	char* binning_buffer;
	char* image_buffer;
	const float* dL_dpix;        /* [3,H,W] */
	float* dL_dmean2D;           /* [P,3]  (.z stays 0); NULL is accepted (a caller that fuses the densification statistics,
	                                stat_* below, has no other use for it) */
	float* dL_dconic;            /* [P,4]  the reference's [P,2,2] (.z = 0); internal to the reference's wrapper
	                                (rasterize_points.cu:152), so NULL is accepted */
	float* dL_dopacity;          /* [P]   */
	float* dL_dcolor;            /* [P,3] */
	float* dL_dmean3D;           /* [P,3] */
	float* dL_dcov3D;            /* [P,6]; NULL is accepted when cov3D_precomp is NULL (the gradient continues into scales and
	                                rotations inside the kernel) */
	float* dL_dsh;               /* [P,M,3] or NULL when shs is NULL */
	float* dL_dscale;            /* [P,3] or NULL when scales is NULL */
	float* dL_drot;              /* [P,4] or NULL when scales is NULL */
	/* Same mask as gsr_forward_args.raw_params (must match the forward call): dL_dopacity / dL_dscale / dL_drot are
	 * then gradients w.r.t. the RAW parameters (chain rule through sigmoid / exp / normalize applied in-kernel). */
	int raw_params;
	/* Extension for keyframe-batch data parallelism (NULL = the reference contract).  [P,3]: when set, dL_dsh is NOT
	 * written (and may be NULL); instead the gradient w.r.t. the SH colour BEFORE the clamp -- dL_dcolor with the
	 * clamped channels zeroed (backward.cu:41-48), zeros for culled Gaussians -- is written here (a VISIBLE Gaussian whose masked
	 * gradient is all zero carries -0.0f in channel 0: numerically nothing, a visibility marker for the lazy rows of
	 * gsr_sh_adam_from_views).  dL_dsh of one view is
	 * basis(dir) x this vector; gsr_sh_grad_from_views rebuilds it for all views after the exchange.  The SH term of
	 * dL_dmean3D is computed as usual. */
	float* dL_dcolor_view;
	/* Extension, optimizer-in-backward for the SH tensor (NULL = the reference contract).  When set, dL_dsh is NOT written
	 * (and may be NULL): the kernel that produces the gradient rows applies this step's Adam update to sh_adam->param (which
	 * must be the same tensor as shs) IN PLACE and to the two moment tensors, for every Gaussian (culled ones with a zero
	 * gradient, as a dense optimizer does) -- the 192 B/Gaussian gradient row never round-trips through HBM.  The rows of
	 * the Gaussians this view culls do not depend on the backward pass at all (zero gradient): gsr_backward updates them on
	 * a second HIP stream it owns, concurrently with the VALU-bound backward blend that leaves HBM nearly idle, and joins
	 * that stream before it returns (environment GSR_SH_ADAM_SIDE_STREAM=0: everything on the caller's stream).  Only for
	 * 16-byte aligned [P,16,3] tensors (GSR_ERR_UNSUPPORTED otherwise).  Together with dL_dcolor_view only in the lazy form
	 * (sh_adam->lazy, window >= 3), and then with another meaning: no step is fused (it follows the exchange:
	 * gsr_sh_adam_from_views); backward runs, on its second stream next to the blend kernel, the rotating catch-up that
	 * bounds the lag of the rows no view lights -- the row blocks b with b % (window - 1) == step % (window - 1) take the
	 * zero-gradient steps they are behind up to step - 1 (what happens AT step is decided by the exchange). */
	const gsr_sh_adam* sh_adam;
	/* Extension (all three or none; NULL = the reference contract): the densification statistics of this view, updated by
	 * the kernel that holds dL_dmean2D in registers instead of a separate pass (gsr_densify_stats, same arithmetic): for
	 * radii > 0: stat_grad_accum += |dL_dmean2D.xy|, stat_denom += 1, stat_max_radii = max(., radii).  [P] floats each. */
	float* stat_grad_accum;
	float* stat_denom;
	float* stat_max_radii;
	/* Extension, optimizer-in-backward for xyz / opacity / scaling / rotation (NULL = the reference contract).  The kernels that
	 * hold these four gradients in registers apply this step's Adam update instead of writing them: dL_dopacity, dL_dscale and
	 * dL_drot are NOT written (and may be NULL), dL_dmean3D is still required but only as scratch between two kernels.  Saves
	 * the 88 B per Gaussian gradient round trip and four optimizer launches.  Needs raw_params == GSR_RAW_OPACITY |
	 * GSR_RAW_SCALING | GSR_RAW_ROTATION (the gradients must be those of the tensors being stepped), scales + rotations (no
	 * cov3D_precomp) and the 16-byte aligned [P,16,3] SH layout (GSR_ERR_UNSUPPORTED otherwise); every Gaussian steps, culled
	 * ones with a zero gradient as a dense optimizer does. */
	const gsr_geom_adam* geom_adam;
	/* Extension for the view-factored exchange (NULL = off; a hipStream_t, consulted only with dL_dcolor_view): dL_dcolor_view is
	 * complete before the last kernel of the backward pass (which only READS it, for the view-direction term of dL_dmean3D).
	 * gsr_backward makes this stream wait for exactly that point, so that a gather the caller issues on it -- the RCCL
	 * all-gather of the exchange -- overlaps that last kernel instead of following the whole pass.  The stream must not be the
	 * one gsr_backward is called with. */
	void* color_view_ready_stream;
	/* Extension for the PACKED view-factored exchange (NULL = off; consulted only with dL_dcolor_view): a message whose prefix and
	 * mask sections gsr_pack_view_plan has filled from this view's radii.  The backward pass writes the seen rows and the header
	 * into it next to dL_dcolor_view -- the message is complete at the same point as the dense view (color_view_ready_stream),
	 * with no pack launch between the backward pass and the gather.  packed_capacity_rows = the rows the buffer has room for
	 * (>= this view's visible count, e.g. P rounded up to 4: the ranks then send the first gsr_packed_view_words(P, max_v K_v)
	 * words).  The same bits as gsr_pack_color_view(P, dL_dcolor_view, campos, packed_capacity_rows, ...). */
	uint32_t* packed_view;
	int packed_capacity_rows;
	/* Extension (NULL = the reference contract): upstream gradients of gsr_forward_args.out_depth / out_alpha, [H,W] each; either
	 * may be NULL (zeros).  The forward pass need not have rendered the maps: the depths and the final transmittance are always
	 * in the buffers of a training forward.  With dD = dL_ddepth, dA = dL_dalpha and S^z_{j+1} the depth blended behind entry j:
	 *   dL/dalpha_j += T_j z_j dD - (S^z_{j+1} dD - T_final dA) / (1 - alpha_j)   (reaches dL_dopacity, dL_dmean2D, dL_dconic,
	 *                                                                              the covariance and scale / rotation)
	 *   dL/dz_j      = sum_p alpha_j T_j dD_p, added to dL_dmean3D through dz/dmean = (view[2], view[6], view[10]).
	 * Colours and SH get nothing from them; dL_dmean2D is the full gradient (so are the fused densification statistics and the
	 * fused Adam steps, geom_adam included). */
	const float* dL_ddepth;
	const float* dL_dalpha;
	/* Extension (all four or none, GSR_ERR_INVALID_ARG otherwise; NULL = the reference contract): gradients of the loss with respect
	 * to the camera -- viewmatrix, projmatrix and campos AS THE KERNELS USE THEM, treated as three independent inputs, with the
	 * conventions of the rest of this pass (consistent with dL_dmean3D: the frustum-clamp rule of computeCov2D, and the depth map's
	 * dL/dz when dL_ddepth is given).  Summed over the Gaussians with radii > 0, x = (mean, 1):
	 *   dL_dviewmatrix[4c+r] = sum dL/dt_r x_c + (J^T dL/dT)(r,c) [c < 3]    t = W2C x, T = J W of the EWA projection, r < 3
	 *   dL_dprojmatrix[4c+r] = sum dL/dhom_r x_c                              hom = Proj x of the pixel position, r = 0, 1, 3
	 *   dL_dcampos           = - sum (the SH view-direction term of dL_dmean3D);  0 with colors_precomp and at D == 0
	 * All 35 floats are written (no zero-fill by the caller); the entries the render does not depend on -- [3], [7], [11], [15] of
	 * dL_dviewmatrix, [2], [6], [10], [14] of dL_dprojmatrix -- are 0, and so is everything for P == 0 or a view that sees nothing.
	 * Nothing here assumes projmatrix = Proj W2C or campos = -R^T t: a caller that built the three from one pose chains the
	 * raw gradients through that construction.  The sums are formed without atomics, in a fixed order: the same inputs give the
	 * same bits.  pose_scratch: gsr_pose_grad_scratch_bytes(P) device bytes, 4-byte aligned, the caller's (contents: don't care).
	 * With geom_adam the sums use the positions as they were before the fused step.  Not together with dL_dcolor_view /
	 * packed_view (the multi-GPU exchange): GSR_ERR_UNSUPPORTED. */
	float* dL_dviewmatrix;       /* [16] device floats, the layout of viewmatrix */
	float* dL_dprojmatrix;       /* [16], the layout of projmatrix */
	float* dL_dcampos;           /* [3] */
	char* pose_scratch;
	/* Extension (NULL = the reference contract): regularisers on the Gaussians this view sees, added to the opacity and scale
	 * gradients inside the pass -- see gsr_geom_reg. */
	const gsr_geom_reg* geom_reg;
	/* Extension (NULL = off: the kernels and arguments of a call without it): absolute screen-space gradients, AbsGS's
	 * "homodirectional" densification statistic (gsplat: absgrad).  [P,2]; every row is written, zeros for culled Gaussians.  With
	 * g_p the contribution of pixel p alone to dL_dmean2D[g] (dL_dmean2D[g] = sum_p g_p),
	 *   dL_dmean2D_abs[g] = (sum_p |g_p.x|, sum_p |g_p.y|)
	 * in the units of dL_dmean2D (the W/2 and H/2 factors included), so that abs >= |dL_dmean2D| componentwise, with equality for a
	 * Gaussian one pixel blends.  dL_ddepth / dL_dalpha count towards it: they are part of dL/dalpha.  The sums are formed per pixel
	 * inside the backward blend (its ABS instantiations) -- they do not factor through the per-Gaussian reduction that dL_dmean2D
	 * takes -- and travel in two spare words of the per-instance slots.  dL_dmean2D itself is unchanged and may still be NULL.
	 * Together with stat_*: stat_grad_accum += the norm of THIS pair instead of |dL_dmean2D.xy|; stat_denom and stat_max_radii as
	 * before.  Works with geom_adam, sh_adam, geom_reg, the pose gradients, GSR_ANTIALIAS and both GSR_BINNING_* arrangements; not
	 * together with dL_dcolor_view / packed_view (the multi-GPU exchange): GSR_ERR_UNSUPPORTED. */
	float* dL_dmean2D_abs;
	/* Extension (read only with GSR_FILTER_3D in raw_params, see there): the filter the forward call was given. */
	const float* filter_3D;      /* [P] */
} gsr_backward_args;

/* Rasterizer::backward, cuda_rasterizer/rasterizer_impl.cu:340-433.
 * Unlike the reference the gradient arrays need NOT be zero-filled by the caller:
 * every element of every non-null output is written (zeros for culled Gaussians),
 * which removes the reference's 300 B/Gaussian torch::zeros pass
 * (src/rasterize_points.cu:149-157).  No host synchronisation. */
int gsr_backward(const gsr_backward_args* args, void* stream);

/* Lazy SH Adam (gsr_sh_adam_lazy): every row of the [P,16,3] tensor takes the zero-gradient steps it is behind, up to and
 * including adam->step = the number of Adam steps the tensor has taken (adam->lr / lr_tail belong to that step, lr_past[k-1] to
 * step - k); afterwards row_step[i] == adam->step for all i and tensor and moments are what the eager update leaves. */
int gsr_sh_adam_flush(int P, const gsr_sh_adam* adam, void* stream);

/* The SH gradient of a keyframe batch from its per-view colour gradients (no counterpart in the reference, which trains
 * on one view per step):   dL_dsh[i][k][ch] = scale * sum_v basis_k(normalize(means3D[i] - campos[v])) * views[v][i][ch]
 * for k < (D+1)^2 and 0 for (D+1)^2 <= k < M; basis_k as computeColorFromSH (forward.cu:20-71).  views is
 * [n_views,P,3] (the dL_dcolor_view outputs of gsr_backward, gathered), campos [n_views,3] on the device; view_stride /
 * campos_stride = floats between consecutive views / centres (0 = dense: 3 P and 3), so that both may live in ONE gathered
 * buffer of [n_views, P + 1, 3] whose last row per view is the camera centre (a single all-gather); scale is 1/n_views
 * for the batch mean.  With one process per GPU this replaces the all-reduce of the [P,M,3] gradient
 * (2 x 192 B sent per Gaussian on a ring) by an all-gather of 12 B per Gaussian and view. */
int gsr_sh_grad_from_views(int P, int D, int M, int n_views, const float* means3D, const float* campos,
                           long long campos_stride, const float* dL_dcolor_views, long long view_stride, float scale,
                           float* dL_dsh, void* stream);

/* The same with the optimizer fused in (as gsr_backward_args.sh_adam): instead of writing dL_dsh, this step's Adam update with
 * that batch-mean gradient is applied to shs [P,16,3] IN PLACE and to the two moment tensors (sh_adam->param must be shs or
 * NULL).  16-byte aligned [P,16,3] tensors only (GSR_ERR_UNSUPPORTED otherwise).  Reads means3D: call it before the
 * positions' own update. */
int gsr_sh_adam_from_views(int P, int D, int M, int n_views, const float* means3D, const float* campos,
                           long long campos_stride, const float* dL_dcolor_views, long long view_stride, float scale,
                           float* shs, const gsr_sh_adam* sh_adam, void* stream);
/* With sh_adam->lazy set (gsr_sh_adam_lazy) the data-parallel step is as lean as the single-GPU one: a row whose colour
 * gradient is zero in EVERY gathered view would take a zero-gradient step -- it is left alone and steps later; a row some view
 * lights first takes the zero-gradient steps it is behind (this rank's forward pass only caught up the rows ITS view sees),
 * then this step, and row_step[i] = step.  1152 B of optimizer traffic per Gaussian some view of the batch sees instead of
 * per Gaussian.  The call may cover a row range (pointers offset by the caller, row_step too).  The lag of the rows nobody
 * lights is bounded either by gsr_backward (sh_adam together with dL_dcolor_view: the catch-up runs ahead of the exchange,
 * next to the blend kernel -- what both hosts do) or by gsr_sh_adam_lazy_slice over ALL rows after the last range of the
 * step (this step's 1/window of the row blocks catches up to `step`).  Same contract as the single-GPU lazy mode otherwise (pass the struct to
 * gsr_forward_args.sh_adam of the step; gsr_sh_adam_flush before anything else touches the tensor); results bit-identical to
 * the eager update (tests/test_lazy_sh_adam.py). */
/* PACKED exchange of the colour gradients.  Most rows of a view's [P,3] colour gradient are all-zero words (a view sees about
 * half of a 2 M-Gaussian map; the culled rest is zero), so a rank may send only the rows its view SEES (lit, or carrying the
 * -0.0f visibility marker) -- the same information in (1 bit + 1/16 word) per Gaussian + 12 B per seen Gaussian:
 *
 *   message (uint32 words; gsr_packed_view_words(P, capacity)):
 *     [0] K = seen rows   [1] P   [2] capacity (rows)   [3] 1 if K > capacity (rows beyond it were DROPPED: a caller's bug)
 *     [4..6] the view's camera centre (3 floats)   [7] 0
 *     prefix[ceil(P/64)]   seen rows in front of the 64-row group (exclusive)
 *     mask  [2 ceil(P/64)] bit (i % 64) of the 64-bit word i / 64: row i is seen (low word first)
 *     rows  [3 capacity]   the seen rows in index order (floats)
 *
 * gsr_pack_color_view builds one message from a view's dL_dcolor_view (four launches; scratch = gsr_pack_scratch_bytes(P));
 * `capacity` must be the same on every rank (the messages travel through ONE all-gather of equal chunks): the ranks agree on
 * max_v K_v beforehand -- K of a view is its number of visible Gaussians, which gsr_forward leaves for the calling thread in
 * gsr_last_visible_count().  gsr_sh_grad_from_packed_views / gsr_sh_adam_from_packed_views are gsr_sh_grad_from_views /
 * gsr_sh_adam_from_views on n_views such messages, msg_stride words apart: bit-identical results (the same rows, the same
 * order of the views).  At 2 M Gaussians, 47 % seen: 11.7 MB instead of 24 MB per rank on every link.
 * gsr_pack_view_plan writes the sections that do not depend on the gradient -- masks and prefix, from the radii of the forward
 * pass (seen = radii > 0; three launches, any stream once gsr_forward has returned) -- so that gsr_backward can write rows and
 * header itself (gsr_backward_args.packed_view). */
size_t gsr_packed_view_words(int P, int capacity_rows);
int gsr_pack_view_plan(int P, const int* radii, uint32_t* message, void* scratch, void* stream);
size_t gsr_pack_scratch_bytes(int P);
int gsr_pack_color_view(int P, const float* dL_dcolor_view, const float* campos, int capacity_rows, uint32_t* message, void* scratch,
                        void* stream);
int gsr_sh_grad_from_packed_views(int P, int D, int M, int n_views, const float* means3D, const uint32_t* messages,
                                  long long msg_stride, float scale, float* dL_dsh, void* stream);
int gsr_sh_adam_from_packed_views(int P, int D, int M, int n_views, const float* means3D, const uint32_t* messages,
                                  long long msg_stride, float scale, float* shs, const gsr_sh_adam* sh_adam, void* stream);
/* Gaussians with radii > 0 in the last gsr_forward of the calling thread (-1 before the first; 0 after a call with P == 0) */
int gsr_last_visible_count(void);
/* 1 if the last gsr_forward of the calling thread had GSR_FORWARD_ONLY set, 0 if not, -1 before the first call */
int gsr_last_forward_only(void);
/* Diagnostic: forward passes of the calling thread whose depth sort ran a second time.  The depth sort takes three passes over 27
 * bits of (key - bits(0.2f)) -- every visible Gaussian has z > 0.2 -- and the host learns the largest key of the view with the
 * instance count; a view with a Gaussian at z >= 13 107 (or a depth that is not a number) is sorted again on all 32 bits.  The
 * results are the same either way; the second path costs about 0.15 ms at 2 M Gaussians. */
long long gsr_depth_resort_count(void);
/* Introspection: the binning arrangement gsr_forward takes for a view of this size with these raw_params bits (1 = tile-first,
 * 0 = depth-first; GSR_BINNING_* above, the GSR_BINNING environment override included). */
int gsr_binning_tile_first(int raw_params, int P, int width, int height);
/* The loud form of the decoders' silent guards (they decode nothing from a message whose P differs and read no row beyond the
 * rows a message holds): copies the n_views headers to the host, WAITS for `stream`, and returns GSR_ERR_INVALID_ARG unless
 * every message says P rows total, K <= min(its own capacity, `capacity_rows` = the rows that travelled) and "nothing dropped".  A synchronisation: for
 * tests, the first steps of a session and a debugging run -- not for every step. */
int gsr_check_packed_views(int P, int n_views, const uint32_t* messages, long long msg_stride, int capacity_rows, void* stream);
/* Diagnostic: the time the calling thread has spent BLOCKED in gsr_forward's one host synchronisation (the read of the instance
 * count behind the projection kernel) and the number of such waits, since the last reset.  A host that runs ahead of the device
 * waits there for most of a step; a wait near zero means the device is waiting for the HOST (launch-bound step: the gaps
 * between kernels are then host time, and every host-side call of the step costs step time). */
int gsr_host_wait_stats(double* total_us, long long* calls, int reset);

/* ahead == 0: after the last gsr_sh_adam_from_views range of the step -- row blocks b with b % window == step % window, every
 * row that is behind catches up to `step`.  ahead != 0 (window >= 3): BEFORE the step's gsr_sh_adam_from_views calls (what
 * gsr_backward does on its second stream in the view-factored mode) -- row blocks b with b % (window - 1) == step % (window - 1)
 * catch up to step - 1.  A step uses one of the two. */
int gsr_sh_adam_lazy_slice(int P, const gsr_sh_adam* adam, int ahead, void* stream);

/* Rasterizer::markVisible, cuda_rasterizer/rasterizer_impl.cu:141-153:
 * present[i] = (view-space z of means3D[i] > 0.2).  present is [P] bytes (bool). */
int gsr_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/* SimpleKNN::knn, third_party/simple-knn/simple_knn.cu:185-221: meanDists[i] = mean of
 * the squared distances from points[i] to its 3 nearest other points.  The reference
 * cudaMalloc's internally; here scratch comes from the callback like everything else. */
int gsr_knn_mean_dist2(int P, const float* points, float* meanDists,
                       gsr_alloc_fn scratchBuffer, void* scratch_ctx, void* stream);

/* ---- train-step kernels next to the rasterizer (the largest non-raster costs) ----
 *
 * Masked L1 + SSIM loss of GaussianMapper::trainForOneIteration (src/gaussian_mapper.cpp:692-698,
 * include/loss_utils.h:28-124):  x = rendered * mask;
 *   loss = (1-lambda) * mean|x - gt| + lambda * (1 - mean(ssim_map(x, gt)))    (11x11 window, sigma 1.5)
 * Writes the scalar loss to *loss (device) and dloss/drendered to grad_rendered [3,H,W]; replaces
 * 5 + 10 grouped conv2d of the autograd graph.  mask may be NULL (all ones).
 * scratch: gsr_loss_scratch_bytes(width, height) device bytes. */
size_t gsr_loss_scratch_bytes(int width, int height);
int gsr_l1_ssim_loss(const float* rendered, const float* gt, const float* mask, int width, int height,
                     float lambda_dssim, float* grad_rendered, float* loss, char* scratch, void* stream);

/* The same loss behind a per-keyframe exposure: a [3,4] affine colour map E (row-major, ON THE DEVICE: it is a tensor being
 * optimised, nothing is read on the host) between render and loss, upstream 3DGS's image.permute(1,2,0) @ E[:3,:3] + E[:3,3]:
 *   x_c = (r_0 E[0][c] + r_1 E[1][c] + r_2 E[2][c] + E[c][3]) * mask_c     (summed in this order; gt is not mapped)
 *   loss as above on x;   G_c = dloss/dx_c * mask_c;   grad_rendered_k = sum_c E[k][c] G_c
 *   grad_exposure[k][c] = sum_p r_k(p) G_c(p)  (c < 3),   grad_exposure[c][3] = sum_p G_c(p)     (all 12 written)
 * Three launches, no atomics: the same inputs give the same bits.  With E = eye(3,4) loss and grad_rendered are those of
 * gsr_l1_ssim_loss bit for bit.  scratch: gsr_loss_exposure_scratch_bytes(width, height) device bytes. */
size_t gsr_loss_exposure_scratch_bytes(int width, int height);
int gsr_l1_ssim_loss_exposure(const float* rendered, const float* gt, const float* mask, int width, int height,
                              float lambda_dssim, const float* exposure, float* grad_rendered, float* grad_exposure,
                              float* loss, char* scratch, void* stream);
/* out_c = image_0 E[0][c] + image_1 E[1][c] + image_2 E[2][c] + E[c][3] per pixel of a [3,H,W] image, for evaluation renders of
 * a keyframe that carries an exposure; no clamping; out may be image. */
int gsr_apply_exposure(const float* image, const float* exposure, int width, int height, float* out, void* stream);

/* Depth L1 loss of an RGB-D keyframe against the rendered depth map (gsr_forward_args.out_depth), Photo-SLAM's
 * RGBD.min_depth / RGBD.max_depth as the sensor's valid range:
 *   loss = weight * sum_{valid p} |depth[p] - gt_depth[p]| / (H W),   valid = min_depth < gt_depth[p] < max_depth
 *   grad_depth[p] = weight * sign(depth[p] - gt_depth[p]) * valid / (H W)   (sign(0) = 0; written for every pixel)
 * *loss (device) and grad_depth [H,W] are written; the sum is deterministic (fixed grid, fixed order: two launches).
 * scratch: gsr_depth_loss_scratch_bytes(width, height) device bytes. */
size_t gsr_depth_loss_scratch_bytes(int width, int height);
int gsr_depth_l1_loss(const float* depth, const float* gt_depth, int width, int height, float min_depth, float max_depth,
                      float weight, float* grad_depth, float* loss, char* scratch, void* stream);

/* Monocular depth prior: a relative-depth map q (MiDaS / Depth Anything style) that is right only up to an unknown scale and shift,
 * against the rendered depth map D (sum z alpha T) and alpha map A of one view.  Per pixel p of the [H,W] view:
 *   valid = A >= alpha_min  &&  D > 0  &&  q finite and > 0  &&  (valid == NULL || valid[p] != 0)      (NaN fails every test)
 *   r     = D / A (the expected depth), or A / D with GSR_DEPTH_PRIOR_INVERSE (for affine-invariant inverse-depth networks);
 *           a pixel whose r is not a positive finite float counts as invalid too.  alpha == NULL means A = 1.
 *   n     = the number of valid pixels;  x~ = mean over the valid pixels;  S_x = sqrt(sum_valid (x - x~)^2)
 * Aligned L1 (default):  (s, t) = argmin sum_valid (s q + t - r)^2 in closed form, constants for the gradient;
 *   loss = weight * sum_valid |r - (s q + t)| / (H W)             (the normalisation of gsr_depth_l1_loss: the weights compare)
 *   dloss/dr = weight * sign(r - (s q + t)) / (H W), sign(0) = 0
 * GSR_DEPTH_PRIOR_PEARSON:  loss = weight * (1 - rho), rho the Pearson correlation of r and q over the valid pixels;
 *   dloss/dr_p = -weight * [ (q_p - q~) / (S_q S_r) - rho (r_p - r~) / S_r^2 ]                          (the full gradient)
 * Chain rule: dr/dD = 1/A, dr/dA = -D/A^2; inverse: dr/dD = -A/D^2, dr/dA = 1/D.  grad_depth and grad_alpha [H,W] are written for
 * every pixel, exactly 0 where the pixel is invalid; grad_alpha is NULL exactly when alpha is.
 * fit[4] = {s, t, rho, n} is written on the device in both modes (rho: a quality signal for the caller); nothing is read on the host.
 * Degenerate input: n < 2, or sum (q - q~)^2 <= 1e-12 sum q^2 -- and, in the Pearson mode, the same test on r: the loss is 0, both
 * gradients are all zero, fit = {0, 0, 0, n}.  (Aligned L1 with only r failing the test: s, t and the loss stand, rho = 0.)
 * No NaN or Inf leaves the kernels for any input.
 * The six moment sums (n, q, r, qq, qr, rr), the fit, the residuals and the gradients are formed in fp64 and rounded once; sums run
 * per thread, per workgroup, then over a fixed grid in index order by one workgroup: no atomics, the same bits on every run, and
 * the same bits from the 16-byte path (every pointer 16-byte aligned) and the scalar path.  Four launches (Pearson: three; fit
 * only: two).  With grad_depth == NULL && loss == NULL only fit is written (grad_alpha must be NULL then); otherwise both are given.
 * scratch: gsr_depth_prior_scratch_bytes(width, height) device bytes, 8-byte aligned. */
#define GSR_DEPTH_PRIOR_INVERSE 1
#define GSR_DEPTH_PRIOR_PEARSON 2
typedef struct gsr_depth_prior_args {
	int width, height;
	const float* depth;      /* [H,W] D */
	const float* alpha;      /* [H,W] A, or NULL */
	const float* prior;      /* [H,W] q */
	const uint8_t* valid;    /* [H,W] bytes, or NULL */
	int flags;               /* GSR_DEPTH_PRIOR_* */
	float alpha_min;
	float weight;
	float* grad_depth;       /* [H,W], or NULL together with loss */
	float* grad_alpha;       /* [H,W]; NULL exactly when alpha is */
	float* loss;             /* [1] */
	float* fit;              /* [4] */
} gsr_depth_prior_args;
size_t gsr_depth_prior_scratch_bytes(int width, int height);
int gsr_depth_prior_loss(const gsr_depth_prior_args* args, char* scratch, void* stream);
/* The prior in the units of the render it was fitted to: out = s q + t, or 1 / (s q + t) with GSR_DEPTH_PRIOR_INVERSE (the flag the
 * fit was made with), from fit[4] on the device; 0 where q is not finite and positive or the result is not a positive finite float.
 * out_depth may be prior.  The map gsr_seed_select / gsr_seed_emit take as gt_depth. */
int gsr_depth_prior_apply(const float* prior, const float* fit, int flags, int width, int height, float* out_depth, void* stream);

/* One torch::optim::Adam step (no amsgrad / weight decay; src/gaussian_model.cpp:477-510 uses eps 1e-15)
 * on a flat fp32 tensor: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= (lr / (1-b1^step)) * m / (sqrt(v) / sqrt(1-b2^step) + eps).  The hyper-parameters are double as in
 * torch::optim::AdamOptions; the scalars derived from them (step size, 1-beta, 1/sqrt(bias correction 2)) are formed in
 * double and rounded once, the element arithmetic is fp32 (pinned to the reference's own trainingSetup +
 * torch::optim::Adam::step, tests/test_densify_reference.py).
 * period/split/lr_tail: if period > 0, elements [split, period) of every period-element row use lr_tail
 * (features_dc and features_rest live in one [P,16,3] buffer with learning rates lr and lr/20). */
int gsr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr,
                  double beta1, double beta2, double eps, int step, int period, int split, double lr_tail, void* stream);

/* The same step for several tensors in ONE launch (the four small per-Gaussian tensors of a data-parallel step, whose
 * gradients arrive together from one all-reduce): element arithmetic exactly as gsr_adam_step, one learning rate and step
 * counter per tensor.  count <= 8; tensors with n == 0 are skipped. */
typedef struct gsr_adam_multi_tensor {
	float* param;            /* UPDATED IN PLACE */
	const float* grad;
	float* exp_avg;
	float* exp_avg_sq;
	long long n;             /* elements */
	double lr;
	int step;                /* >= 1: the step being taken */
	float grad_scale;        /* the gradient is multiplied by this as it is read (1 = as it is): the 1/N of a batch mean whose
	                            all-reduce SUMMED -- one pass over the gradients less than averaging first */
} gsr_adam_multi_tensor;
int gsr_adam_step_multi(int count, const gsr_adam_multi_tensor* tensors, double beta1, double beta2, double eps, void* stream);

/* Per-view densification statistics (src/gaussian_mapper.cpp:714-719, src/gaussian_model.cpp:817-831) for
 * vis = radii > 0:  max_radii2D = max(max_radii2D, radii); xyz_gradient_accum += |dL_dmean2D.xy|; denom += 1.
 * dL_dmean2D is the [P,3] viewspace gradient; accum/denom are [P] ([P,1]) floats, max_radii2D [P] floats. */
int gsr_densify_stats(int P, const float* dL_dmean2D, const int* radii, float* xyz_gradient_accum, float* denom,
                      float* max_radii2D, void* stream);
/* The same from the absolute pair (gsr_backward_args.dL_dmean2D_abs, [P,2]): xyz_gradient_accum += |dL_dmean2D_abs| -- for a caller
 * that keeps the statistics pass apart from the backward pass.  The bits of the fused form (stat_* next to dL_dmean2D_abs). */
int gsr_densify_stats_abs(int P, const float* dL_dmean2D_abs, const int* radii, float* xyz_gradient_accum, float* denom,
                          float* max_radii2D, void* stream);

/* ---- densification / pruning as stream compaction ----
 * GaussianModel::densifyAndPrune = densifyAndClone + densifyAndSplit (N = 2) + the final prunePoints
 * (src/gaussian_model.cpp:716-815) rebuild every tensor and Adam moment 4-6 times through boolean-mask indexing and cat.
 * Here: gsr_densify_select turns the per-Gaussian decisions into a gather plan with deterministic ballot/prefix ranks (no
 * atomics, no host round trip inside), the caller reads the six counts ONCE to size the new tensors, and
 * gsr_densify_gather rebuilds all five parameter tensors, their ten moment tensors and the statistics in one launch.
 * Order of the new set, as the reference's: [originals neither split nor pruned | surviving clones | surviving first
 * children | surviving second children], each block in source order.
 *
 * Decisions (all fp32, thresholds formed as the reference forms them):
 *   g = accum / denom, nan -> 0;  smax = max(exp(scaling));  big = smax > percent_dense * extent
 *   clone: sqrt(g*g) >= max_grad && !big          split: g >= max_grad && big
 *   pruned row: sigmoid(opacity) < min_opacity || (max_screen_size != 0 && its activated scale > 0.1f * extent)
 *   (clones inherit the source's decision; both children carry scale / 1.6; max_radii2D is zero at that point -- it was
 *   reset by densificationPostfix -- so the reference's screen-size term never fires)
 * prune_mask != NULL selects GaussianModel::prunePoints(mask) (:588-642) instead: keep = !mask, no clones, no children. */
typedef struct gsr_densify_select_args {
	int P;
	const float* xyz_gradient_accum;  /* [P] ([P,1]) */
	const float* denom;               /* [P] */
	const float* scaling;             /* [P,3] log-scales (the raw parameter) */
	const float* opacity;             /* [P] logits (the raw parameter) */
	float percent_dense, max_grad, min_opacity, extent;
	int max_screen_size;
	const uint8_t* prune_mask;        /* [P] bytes (bool) or NULL */
} gsr_densify_select_args;
size_t gsr_densify_scratch_bytes(int P);
/* counts: DEVICE int[8], written on the stream: [0] kept originals, [1] surviving clones, [2] surviving parents of
 * children (2 rows each), [3] split-selected parents k (the reference draws 2k x 3 normal samples, parent-major per copy),
 * [4] clone-selected, [5] rows of the new set = [0] + [1] + 2 [2].  scratch: gsr_densify_scratch_bytes(P) device bytes; it
 * holds the plan and must reach gsr_densify_gather unchanged. */
int gsr_densify_select(const gsr_densify_select_args* args, char* scratch, int* counts, void* stream);

typedef struct gsr_densify_gather_args {
	int P;                            /* rows of the source arrays (as passed to gsr_densify_select) */
	int n_new, n_keep, n_clone, n_child, n_split;   /* counts[5], [0], [1], [2], [3] read back by the caller */
	int features_row_floats;          /* 3 * M of the [P,M,3] SH tensor */
	/* index 0..4 = xyz [.,3], features [.,M,3], opacity [.,1], scaling [.,3], rotation [.,4]; moments may be NULL (in and
	 * out together) when no optimizer state exists.  In and out must not overlap. */
	const float* param_in[5];
	const float* exp_avg_in[5];
	const float* exp_avg_sq_in[5];
	float* param_out[5];
	float* exp_avg_out[5];
	float* exp_avg_sq_out[5];
	/* [2 n_split, 3] STANDARD normal draws: a child's offset is R(q_parent) * (z * exp(scaling_parent)), i.e.
	 * at::normal(0, std) of the reference (:731-736) is randn * std.  NULL allowed when n_child == 0. */
	const float* samples;
	float* stats_out[3];              /* xyz_gradient_accum, denom, max_radii2D of the new set ([n_new] each): zero-filled; NULL = skip */
	/* GaussianModel::exist_since_iter_ ([P] / [n_new] int32; both or neither): every row of the new set inherits its source's
	 * value -- prunePoints (:636), clones (:782) and split children (:744) alike */
	const int* exist_since_iter_in;
	int* exist_since_iter_out;
	/* Extension (NULL = the reference's row order: kept originals, clones, first children, second children, each in source order):
	 * gsr_densify_morton_scratch_bytes(n_new) device bytes -- the rows of the new set are then laid out along a Z-order curve of
	 * their (parents') positions.  The SAME Gaussians with the same values, moments, statistics and exist_since_iter, in another
	 * order (a view's depth ties then resolve by the new ids).  Why: every per-Gaussian kernel of a step fetches the rows of the
	 * Gaussians a view sees, a spatially compact subset; when neighbours in space are neighbours in memory those rows share 128-byte
	 * lines instead of being a random half of every line (measured on the synthetic cloud, whose ids carry no locality at all:
	 * -5 % of the train step; a SLAM map that grows keyframe by keyframe has some of it by construction).  The gather rewrites every
	 * tensor anyway: the order is free. */
	char* morton_scratch;
} gsr_densify_gather_args;
size_t gsr_densify_morton_scratch_bytes(int n_new);
int gsr_densify_gather(const gsr_densify_gather_args* args, const char* scratch, void* stream);

/* ---- fixed-budget maps: 3DGS-MCMC relocation, growth and position noise (Kheradmand et al. 2024) ----
 * The other half of the method whose opacity / scale L1 terms are gsr_geom_reg: instead of cloning and splitting by a gradient
 * threshold, dead Gaussians (sigmoid(opacity) <= min_opacity) are re-spawned on live ones drawn in proportion to their
 * opacity, the model grows by 5 % per event up to a cap, and every step adds covariance-shaped noise to the positions.  The
 * row count never changes on a relocation, so no tensor is rebuilt: gsr_mcmc_relocate works IN PLACE on the five raw
 * parameter tensors and their ten Adam moments.  No host synchronisation, no floating-point atomics; the same inputs give
 * the same bits on every run.
 *
 *   o_i = sigmoid(opacity_i) in fp32 (as gsr_densify_select forms it);  row i is dead iff o_i <= min_opacity
 *   w_i = (uint32) lrintf(o_i * 2^24);  relocating (n_add == 0): w_i = 0 for dead rows;  growing: every row keeps its weight
 *         (upstream's add_new_gs samples over all rows)
 *   C   = inclusive prefix sum of w in uint64 (exact, independent of order)
 *   destinations: relocating, the dead rows in index order, the k-th takes draws[k]; dead rows of rank >= n_draws stay as
 *         they are.  Growing, row P + k takes draws[k], k < n_add.
 *   source of a draw u: t = min((uint64)((double)u * (double)C[P-1]), C[P-1] - 1), the first s with C[s] > t.
 *         C[P-1] == 0: nothing moves.
 *   N_s = 1 + number of draws that chose s, capped at 51 in the formulas:
 *         o'     = 1 - (1 - o_s)^(1/N), clamped to [min_opacity, 1 - 2^-24]
 *         D      = sum_{i=1..N} sum_{k=0..i-1} C(i-1,k) (-1)^k o'^(k+1) / sqrt(k+1)          (both formed in double)
 *         scale' = exp(scaling_s) * o_s / D
 *   every source with N_s > 1 and every destination of it store opacity = logit(o'), scaling = log(scale'); a destination
 *   also copies xyz, the SH row and the rotation of its source and inherits its exist_since_iter, and its three statistics
 *   are zeroed.  The moments of all five tensors are zeroed at every destination and at every source with N_s > 1.
 *   Every other row of every array is left untouched. */
typedef struct gsr_mcmc_relocate_args {
	int P;                      /* live rows */
	int n_add;                  /* 0 = relocate; > 0 = grow: rows [P, P + n_add) of EVERY array below are destinations (the
	                               caller guarantees the room) */
	int n_draws;                /* >= n_add */
	int features_row_floats;    /* 3 * M of the [.,M,3] SH tensor */
	float min_opacity;          /* in (0, 1); 0.005 in both hosts */
	/* index 0..4 = xyz [.,3], features [.,M,3], opacity [.,1], scaling [.,3], rotation [.,4] (the raw parameters), UPDATED IN
	 * PLACE; the moments may be NULL, all ten together, when no optimizer state exists */
	float* param[5];
	float* exp_avg[5];
	float* exp_avg_sq[5];
	const float* draws;         /* [n_draws] uniform draws in [0, 1): the caller's, like samples of gsr_densify_gather */
	int* exist_since_iter;      /* optional [.] int32 */
	float* stats[3];            /* optional xyz_gradient_accum, denom, max_radii2D ([.] each); NULL = skip */
	uint32_t* out_weights;      /* optional [P]: exactly the weights used */
} gsr_mcmc_relocate_args;
size_t gsr_mcmc_scratch_bytes(int P, int n_draws);
/* counts: DEVICE int[8], written on the stream: [0] dead rows, [1] destinations written, [2] distinct sources with N > 1,
 * [3] the largest N (uncapped; 0 when nothing moved), the rest zero.  scratch: gsr_mcmc_scratch_bytes(P, n_draws) device
 * bytes.  P == 0 writes zeros to counts and nothing else. */
int gsr_mcmc_relocate(const gsr_mcmc_relocate_args* args, char* scratch, int* counts, void* stream);

/* The position noise of 3DGS-MCMC's Langevin step, on the raw parameters, one launch:
 *   o_i = sigmoid(opacity_i);  g_i = 1 / (1 + expf(100 * (o_i - 0.005)))   (upstream's sigmoid(100 * ((1 - o) - 0.995)); an
 *         opaque Gaussian gets exactly 0: the exponential overflows to +inf and the quotient stays finite)
 *   Sigma_i = R(q_i) diag(exp(scaling_i)^2) R(q_i)^T, q normalised as under GSR_RAW_ROTATION, built as gsr_forward builds it
 *   xyz_i += Sigma_i * (z_i * (g_i * noise_scale))
 * z: [P,3] STANDARD normal draws, the caller's.  xyz is UPDATED IN PLACE. */
int gsr_mcmc_add_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* z,
                       float noise_scale, void* stream);

/* ---- seeding Gaussians from an RGB-D frame where the map does not explain it (SplaTAM's add_new_gaussians, MonoGS's
 * unexplored-region insertion) ----
 * gsr_seed_select compares the alpha and depth maps of a forward-only render of the current map (gsr_forward_args.out_alpha /
 * out_depth) with the sensor depth, ranks the unexplained pixels and leaves the plan in scratch; the caller reads counts[0] ONCE,
 * makes room, and gsr_seed_emit back-projects the planned pixels and writes them as rows [P, P + n_emit) of the five raw parameter
 * tensors, IN PLACE.  No host synchronisation inside, no atomics on global memory, no floating-point sum: the same inputs give
 * the same bits on every run, and every decision is an fp32 comparison that numpy restates exactly.
 *
 * Selection (pixel p = v * width + u, all values fp32; a = alpha[p], d = depth[p], both 0 when the maps are NULL; g = gt_depth[p]):
 *   valid     = min_depth < g && g < max_depth                      (the rule of gsr_depth_l1_loss: NaN, inf and 0 fail it)
 *   candidate = u % stride == offset_x && v % stride == offset_y
 *   unseen    = a < alpha_threshold
 *   e         = |g - d|
 *   T         = max(depth_error_abs, depth_error_median_factor * median)   (one fp32 product, one fp32 max); the factor 0 leaves
 *               T = depth_error_abs and no median is formed; both 0 switch the depth rule off
 *   in front  = d > g && e > T                                      (the map puts a surface in front of the measured one)
 *   selected  = candidate && valid && (unseen || in front)
 * Median: the exact LOWER median of e over ALL valid pixels (candidates or not), the element of ascending rank (n_valid - 1) / 2.
 *   Non-negative floats order like their bit patterns: a radix select, four passes of eight bits over per-workgroup histograms
 *   (integer counts, summed per bin in workgroup order) -- no sort, no host read.
 * Order: the selected pixels are ranked in row-major pixel order (block scan of the per-thread counts, an exclusive scan of the
 *   block totals); r below is that rank.
 * Thinning (n_emit < n_selected): the selected pixel of rank r is written iff floor((r+1) n_emit / n_selected) > floor(r n_emit /
 *   n_selected) (uint64), to row P + floor(r n_emit / n_selected) -- an even thinning over the image, not a truncation of its top.
 *   Row P + j therefore holds the pixel of rank ceil((j+1) n_selected / n_emit) - 1.
 * A written row, z = gt_depth[p]:
 *   p_c      = ((u - cx) * z / fx, (v - cy) * z / fy, z)            (the operation order of gsr_reproject_depth_pinhole)
 *   xyz      = R^T (p_c - t), R[r][c] = viewmatrix[4c+r], t[r] = viewmatrix[12+r]   (world -> camera, rigid)
 *   scaling  = logf(scale_factor * stride * z / (0.5f * (fx + fy))) three times: the pixel's footprint at its depth (SplaTAM's
 *              isotropic rule; no kNN -- the spacing of a pixel grid is known)
 *   rotation = (1, 0, 0, 0);   opacity = logit(init_opacity), formed on the host in double and rounded once
 *   SH row   = ((c - 0.5f) / 0.28209479177387814f for the three channels c of image at p, then zeros); image NULL: all zeros
 *   the ten moment rows 0, exist_since_iter = iteration, the three statistics 0, out_pixel = p.
 *   Nothing outside rows [P, P + n_emit) is touched. */
typedef struct gsr_seed_select_args {
	int width, height;
	const float* alpha;      /* [H,W] out_alpha of a render of the current map; NULL = no map yet: 0 everywhere */
	const float* depth;      /* [H,W] out_depth (sum z alpha T, NOT normalised); NULL together with alpha */
	const float* gt_depth;   /* [H,W] sensor depth */
	float min_depth, max_depth;
	float alpha_threshold;           /* SplaTAM 0.5 */
	float depth_error_abs;
	float depth_error_median_factor; /* SplaTAM 50 */
	int stride, offset_x, offset_y;  /* stride >= 1, offsets in [0, stride) */
} gsr_seed_select_args;
size_t gsr_seed_scratch_bytes(int width, int height);
/* counts: DEVICE int[8], written on the stream: [0] selected, [1] of them by the unseen rule, [2] by the depth rule alone, [3] valid
 * pixels, [4] the bits of the median (0 if unused or no valid pixel), the rest 0.  scratch: gsr_seed_scratch_bytes(width, height)
 * device bytes; it holds the plan and must reach gsr_seed_emit unchanged.  The three maps are read with 16-byte loads when all
 * their bases are 16-byte aligned, with 4-byte loads otherwise.  width * height == 0 writes zeros to counts and nothing else;
 * stride < 1, an offset outside [0, stride), alpha and depth not both NULL or both set: GSR_ERR_INVALID_ARG. */
int gsr_seed_select(const gsr_seed_select_args* args, char* scratch, int* counts, void* stream);

typedef struct gsr_seed_emit_args {
	int width, height, stride;   /* as passed to gsr_seed_select */
	int n_selected, n_emit;      /* counts[0] read back; 0 <= n_emit <= n_selected rows are written */
	int P;                       /* rows [P, P + n_emit) of every array below are the destinations (the caller guarantees the room) */
	int features_row_floats;     /* 3 * M of the [.,M,3] SH tensor */
	const float* gt_depth;
	const float* image;          /* [3,H,W] or NULL (DC = 0) */
	const float* viewmatrix;     /* DEVICE [16], element (r,c) at [4c+r], world -> camera, rigid: the one gsr_forward takes */
	float fx, fy, cx, cy;
	float scale_factor, init_opacity;   /* init_opacity in (0, 1) */
	/* index 0..4 = xyz [.,3], features [.,M,3], opacity [.,1], scaling [.,3], rotation [.,4] (the raw parameters); the moments may
	 * be NULL, all ten together, when no optimizer state exists */
	float* param[5];
	float* exp_avg[5];
	float* exp_avg_sq[5];
	int* exist_since_iter;       /* optional [.] int32 */
	int iteration;
	float* stats[3];             /* optional xyz_gradient_accum, denom, max_radii2D ([.] each); NULL = skip */
	int* out_pixel;              /* optional [n_emit]: v * width + u of every written row */
} gsr_seed_emit_args;
/* width * height == 0 or n_emit == 0 writes nothing and returns GSR_OK.  stride < 1, init_opacity outside (0, 1), n_emit > n_selected:
 * GSR_ERR_INVALID_ARG. */
int gsr_seed_emit(const gsr_seed_emit_args* args, const char* scratch, void* stream);

/* ---- Photo-SLAM's point-cloud kernels ----
 * transformPoints (src/operate_points.cu:73-93): out = M[:3,:4] * (p, 1), M = transformmatrix[16] with
 * element (r,c) at [4c+r] (transformPoint4x3). */
int gsr_transform_points(int P, const float* points, const float* transformmatrix, float* out_points, void* stream);
/* scale_and_transform_points (src/operate_points.cu:52-71): for mask[i] != 0: out_points[i] = M * (scale * p_i),
 * out_rots[i] = quaternion of (M[:3,:3] * R(q_i)), q stored (w, x, y, z).  Unmasked rows are NOT written.
 * reference_rot_layout != 0 reproduces insert_rot_to_rots exactly as shipped (cuda_rasterizer/operate_points.h:
 * 175-178 writes component +2 twice and never +3: the row becomes (w, x, z, <previous content>)); 0 writes the
 * intended (w, x, y, z). */
int gsr_scale_transform_points(int P, float scale, const float* points, const float* rots, const float* transformmatrix,
                               const uint8_t* mask, float* out_points, float* out_rots, int reference_rot_layout,
                               void* stream);
/* reproject_depths_pinhole (src/stereo_vision.cu:39-61): pixel i = (u = i % width, v = i / width), for mask[i]:
 * out = ((u-cx)*d/fx, (v-cy)*d/fy, d).  Unmasked rows are NOT written. */
int gsr_reproject_depth_pinhole(int P, int width, float fx, float fy, float cx, float cy, const float* depths,
                                const uint8_t* mask, float* out_points, void* stream);
/* search_neighborhood_to_estimate_depth_and_reproject_pinhole (src/stereo_vision.cu:63-136): keypoints with a 3D
 * point are copied; the others take the depth of the nearest (squared pixel distance <= max_pixel_dist, first wins)
 * keypoint that has one and are re-projected, or get z = -1.  colors is indexed exactly as the reference does
 * (colors[int(v*width+u) + 0..2]). */
int gsr_neighborhood_depth_pinhole(int N, int width, float fx, float fy, float cx, float cy, float max_pixel_dist,
                                   const float* pixels, const uint8_t* has3D, const float* point3D, const float* colors,
                                   float* out_points, float* out_colors, void* stream);

/* ---- the 3-D smoothing filter of GSR_FILTER_3D from the keyframes (Mip-Splatting's compute_3D_filter) ----
 * cameras: K structs ON THE DEVICE; viewmatrix as gsr_forward_args.viewmatrix, focal lengths and size in pixels of the finest level
 * the keyframe is trained at.  Per Gaussian and camera, in float32, every operation rounded on its own, in this order:
 *   1. (x, y, z) = the view-space point, x = V[0] X + V[4] Y + V[8] Z + V[12] (summed left to right), y and z likewise; z is
 *      exactly the expression gsr_forward culls by, so z > 0.2f is the rasterizer's own near test
 *   2. u = (x / z) * focal_x + 0.5f * width,  v = (y / z) * focal_y + 0.5f * height
 *   3. the camera OBSERVES the Gaussian iff z > 0.2f and -0.15f width <= u <= 1.15f width and -0.15f height <= v <= 1.15f height
 *      (Mip-Splatting's 15 % margin)
 *   4. T_i = min over the observing cameras of z / fmaxf(focal_x, focal_y)
 *   5. filter_3D[i] = sqrtf(variance) * T_i                                    (variance: 0.2f upstream)
 *   6. a Gaussian no camera observes gets sqrtf(variance) * max over the observed Gaussians of T_i (upstream's rule); when nothing
 *      is observed, or K == 0, every entry is 0
 *   7. P == 0 writes nothing
 * This differs from upstream in two ways: upstream takes the smallest z and the globally largest focal length separately, and
 * projects both axes with focal_x.  For cameras of one focal length and square pixels the two definitions coincide; with pyramid
 * levels of different focal lengths this one is the exact per-camera sampling interval z / f.
 * The maximum of step 6 is formed without float atomics (per-workgroup maxima in `scratch`, a second small launch): the same inputs
 * give the same bits on every run.  scratch: gsr_filter3d_scratch_bytes(P) device bytes, 4-byte aligned, contents don't care.
 * GSR_ERR_INVALID_ARG: P or K negative, a negative or non-finite variance, a NULL pointer (cameras may be NULL when K == 0). */
typedef struct gsr_filter3d_camera {
	float viewmatrix[16];
	float focal_x, focal_y, width, height;
} gsr_filter3d_camera;   /* 80 bytes */
size_t gsr_filter3d_scratch_bytes(int P);
int gsr_filter3d_compute(int P, const float* means3D, int K, const gsr_filter3d_camera* cameras, float variance, float* filter_3D,
                         char* scratch, void* stream);

/* Scratch sizes (bytes) gsr_forward will request, for callers that pre-allocate. */
size_t gsr_geometry_bytes(int P);
size_t gsr_binning_bytes(int num_rendered);
size_t gsr_image_bytes(int width, int height);
/* ... for a call with these raw_params bits: with GSR_FORWARD_ONLY the smaller layouts of that mode, otherwise the two above */
size_t gsr_binning_bytes_for(int num_rendered, int raw_params);
size_t gsr_image_bytes_for(int width, int height, int raw_params);
size_t gsr_knn_scratch_bytes(int P);
size_t gsr_pose_grad_scratch_bytes(int P);   /* gsr_backward_args.pose_scratch */
size_t gsr_geom_reg_scratch_bytes(int P);    /* gsr_geom_reg.scratch */

/* Optional per-stage timing with HIP events recorded on the caller's stream (process-wide switch,
 * meant for single-stream benchmarking).
 * After gsr_profile_enable(1), every gsr_forward / gsr_backward records events between its
 * stages; gsr_profile_read() waits for the last ones and returns milliseconds per stage
 * (-1 for stages that did not run or were not timed), indexed 0..gsr_profile_stage_count()-1.
 * gsr_profile_enable(2) times only the backward blend (two event records per step instead of
 * eleven: every record is a ~5 us bubble in the stream); gsr_profile_enable(0) switches off. */
int gsr_profile_enable(int on);
int gsr_profile_stage_count(void);
const char* gsr_profile_stage_name(int stage);
int gsr_profile_read(float* ms, int count);

const char* gsr_strerror(int status);
/* hipError_t of the last failing HIP call on this thread (0 if none), and its name. */
int gsr_last_hip_error(void);
const char* gsr_last_hip_error_string(void);
/* "hip-gfx950" for the product library. */
const char* gsr_backend(void);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
