/*
 * mad_pm.h -- C ABI of regularised Perona-Malik (nonlinear isotropic) diffusion on the GPU:
 * Perona and Malik's scalar diffusivity on Catte's pre-smoothed gradient, a sibling of the
 * structure-tensor filters of mad_ced.h.  The diffusion tensor g I is derived from the image
 * on the device and handed to the MAD solver of mad.h in place; the implicit steps are stable
 * at time steps of 1-10, where explicit schemes are capped near 0.06-0.125.
 *
 * Definition (image u, spacing h, borders replicated by index clamping, x fastest; K0 / K1 the
 * sampled Gaussian / first-derivative taps of mad_ved.h's FIR operator, radius
 * max(1, ceil(4 sigma / h_d)) on axis d -- the operator of step 1 of mad_ced.h):
 *   1. gradient at the noise scale sigma, exactly mad_ced.h's step 1:
 *        3D: g_d = K1 along d, K0 along the other two axes (passes z, y, x; correlation
 *            sum_t K(t) f(clamp(i + t))), times 1 / h_d once
 *        2D: gx = K1x(K0y u) / hx, gy = K0x(K1y u) / hy (pass along y first, then x)
 *   2. s = gx gx + gy gy (+ gz gz), summed left to right in the storage precision with
 *      contraction off, then taken to fp64
 *   3. diffusivity, fp64 in every precision mode (contrast K, exponent m, 0 < alpha < 1):
 *        MAD_PM_WEICKERT     g0 = 1 - h(s), h(s) = exp(-(K^2 / s)^m) for s > 0, else 0 (the h
 *                            of mad_ced.h: g is EED's across-edge eigenvalue wherever
 *                            mu1 - mu0 = |grad u_sigma|^2)
 *        MAD_PM_EXPONENTIAL  g0 = exp(-s / K^2)       (m is ignored)
 *        MAD_PM_RATIONAL     g0 = 1 / (1 + s / K^2)   (m is ignored)
 *      g = alpha + (1 - alpha) g0
 *   4. D = g I, fp64 SoA [xx,xy,xz,yy,yz,zz] (2D: [xx,xy,yy]): the off-diagonals are exact
 *      0.0, all diagonals hold the same bits
 *   5. outer loop as in CED / VED: per iteration one tensor generation from the current image,
 *      then diffusion_iterations implicit steps of time_step through the MAD solver
 *      (MaxCycles fixed at 100).  The classic semi-implicit scheme is
 *      diffusion_iterations = 1, iterations = n.
 * See DESIGN.md "Nonlinear isotropic diffusion (Perona-Malik)" and tests/pm_numpy.py.
 *
 * Contrast from a quantile (contrast_mode = MAD_PM_CONTRAST_QUANTILE).  K is in units of the
 * image's own gradient; Perona and Malik set it from the data, once per iteration, as the value
 * below which 90 % of the gradient magnitudes lie.  In this mode `contrast` holds that share q,
 * 0 < q <= 1, and every tensor generation finds its K on the device:
 *   rank   with s(p) of step 2 over all N voxels, k = min(N - 1, max(0, (int64)ceil(q (double)N) - 1))
 *          (product and ceil in fp64 on the host), s_q = the k-th smallest s(p), 0-based:
 *          numpy's np.quantile(s, q, method="inverted_cdf").  The selection is exact.
 *   map    step 3 with K^2 := s_q, used as it is (never via sqrt and squaring); the K reported
 *          (mad_pm_stats.contrast_used) is sqrt(s_q).  K^2 stays in device memory between the
 *          selection and the map: a tensor generation has no host synchronisation.
 *   s_q = 0 (a constant image, or more than the share q of the voxels flat): the limit K -> 0+ of
 *          all three diffusivities, g0 = 1 where s = 0 and g0 = 0 elsewhere; K is reported as 0,
 *          a valid result.
 *   In mad_pm_run / mad_pm_run_device every outer iteration selects anew from its iterate.
 * The mode needs N < 2^32 (mad_pm_create refuses more).  Its entry points for inspection,
 * mad_pm_contrast and mad_pm_select, are declared in mad_pm_quantile.h.  See DESIGN.md
 * "Contrast from a quantile" and tests/pm_quantile_numpy.py.
 *
 * Vector-valued images (channels = C > 1; Gerig et al. 1992): one diffusivity from the summed
 * squared gradients of all channels, g(sum_c |grad u_c,sigma|^2), applied to every channel.
 *   layout every image argument of the entry points below is planar: C arrays of
 *          N = size[0] size[1] size[2] elements, channel c at element offset c N, input and output
 *          alike.  channels = 0 is read as 1; anything outside 1..16 is MAD_ERR_INVALID from
 *          mad_pm_create, before a device is touched.
 *   1.     per channel, exactly as above
 *   2.     s_c = gx_c gx_c + gy_c gy_c (+ gz_c gz_c) as above, then s = s_0 + s_1 + ... + s_{C-1},
 *          summed left to right in the storage precision with contraction off, then taken to
 *          fp64.  With C = 1 this is the s of step 2 bit for bit.
 *   3.-4.  on the joint s.  Quantile mode selects among the N values of the joint s, and
 *          contrast_used is sqrt(s_q) of the joint s.
 *   5.     per outer iteration: one tensor generation from all current channels, one solver
 *          setup, then every channel through diffusion_iterations implicit steps with the same
 *          operators.
 *   stats  total_cycles sums over the channels, last_relres is the largest of the channels'
 *          last-step values in the last iteration, stalled the OR over the channels, diffusion_ms
 *          covers all channels; MAD_ERR_NOT_CONVERGED as for one channel.  3D: the z and y passes
 *          alternate per channel, so pass_ms[0] is the first channel's z pass and pass_ms[1] every
 *          pass between it and the x pass.
 *   mad_pm_tensor returns the joint tensor and the joint g; mad_pm_gradient writes C dim arrays of
 *   N, channel slowest and (gx, gy(, gz)) within a channel; mad_pm_contrast gives the joint K;
 *   mad_pm_select is unchanged.  See DESIGN.md "Vector-valued images" and
 *   tests/pm_vector_numpy.py.
 *
 * Limit on sigma.  Every kernel keeps its tile and the taps' halo in 128 KiB of LDS and shrinks
 * the tile for long taps; taps that do not fit the smallest tile make mad_pm_run,
 * mad_pm_tensor and mad_pm_gradient return MAD_ERR_UNSUPPORTED ("Gaussian taps too long for
 * the LDS tiles") before anything is launched; the context stays usable.
 *   3D: the z and y passes are mad_ced.h's and set the limit: radius along z <= 30 in MAD_FP64
 *       (sigma <= 7.5 h_z) and <= 62 with fp32 storage (sigma <= 15.5 h_z); along y <= 62 / 126.
 *       The x pass (three rows of 256 + 2 R) allows far more.
 *   2D: the fused kernel's smallest tile is 16 x 4; with R = (Rx, Ry) it needs
 *       max((16 + 2 Rx)(4 + 2 Ry), 136) + 10 (16 + 2 Rx) elements, which fits for equal radii
 *       R <= 56 in MAD_FP64 (sigma <= 14 h) and R <= 83 with fp32 storage (sigma <= 20.75 h).
 * fp32 storage, the default precision, is the way past the fp64 limits.
 *
 * Monotonicity.  The MAD stencil discretises div(g grad u) as g lap u + grad g . grad u with
 * central differences: the two neighbour weights along an axis are
 * -dt / h^2 (g(p) +- (g(p + 1) - g(p - 1)) / 4).  Where |g(p + 1) - g(p - 1)| <= 4 g(p) they are
 * non-positive and the implicit step obeys the maximum principle at any time step; a diffusivity
 * that drops from 1 to alpha within two grid points (a small sigma and alpha with a contrast far
 * below the edge's gradient) violates it, and the step then over- and undershoots at the edge.
 * A noise scale of 1-2 grid spacings, the rational diffusivity, or a larger alpha keep it
 * ("Monotonicity").
 */
#ifndef MAD_PM_H
#define MAD_PM_H

#include "mad.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mad_pm_diffusivity {
  MAD_PM_WEICKERT = 0,             /* 1 - exp(-(K^2 / s)^m): flat below K, a sharp drop above */
  MAD_PM_EXPONENTIAL = 1,          /* exp(-s / K^2): Perona and Malik's first function */
  MAD_PM_RATIONAL = 2              /* 1 / (1 + s / K^2): Perona and Malik's second function */
} mad_pm_diffusivity;

typedef enum mad_pm_contrast_mode {
  MAD_PM_CONTRAST_ABSOLUTE = 0,    /* contrast is K itself */
  MAD_PM_CONTRAST_QUANTILE = 1     /* contrast is q, 0 < q <= 1: K^2 = the q-quantile of s, per tensor
                                      generation ("Contrast from a quantile" above) */
} mad_pm_contrast_mode;

/* mad_pm_desc.options.  Test only: in MAD_PM_CONTRAST_ABSOLUTE, `contrast` holds K^2 itself, fed to
 * the map unsquared, so a test can give the fused kernel the very bits a selection returned. */
#define MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED 0x80000000u

typedef struct mad_pm_desc {
  uint32_t abi_version;            /* MAD_ABI_VERSION */
  int64_t size[3];                 /* x, y, z (dim 2: z = 1) */
  double spacing[3];               /* image spacing, x first (dim 2: spacing[2] is ignored) */
  int32_t diffusivity;             /* mad_pm_diffusivity, MAD_PM_WEICKERT */
  double noise_scale;              /* sigma, physical units, 0.5 */
  double contrast;                 /* K, 1.0 (MAD_PM_CONTRAST_QUANTILE: the share q) */
  double exponent;                 /* m, 2.0 (MAD_PM_WEICKERT only) */
  double alpha;                    /* 0 < alpha < 1, 0.01 */
  uint32_t iterations;             /* 1  (outer iterations: tensor generation + diffusion) */
  uint32_t diffusion_iterations;   /* 5  (MAD NumberOfSteps per iteration) */
  /* MAD parameters of the diffusion steps (MaxCycles fixed at 100, as in CED / VED) */
  int32_t cycle;                   /* MAD_VCYCLE */
  double time_step;                /* 0.1 */
  double tolerance;                /* 1e-6 */
  uint32_t diffusion_iterations_per_grid; /* 2 */
  int32_t smoother;                /* mad_smoother, MAD_GAUSS_SEIDEL */
  int32_t precision;               /* MAD_PRECISION_AUTO (default) / MAD_FP32 / MAD_FP32_REFINE: fp32
                                      passes, the diffusion solve as mad_create resolves it;
                                      MAD_FP64: fp64 throughout.  The diffusivity runs in fp64
                                      in every mode. */
  int32_t device;                  /* HIP device, -1 = current */
  int32_t verbose;                 /* 0 */
  uint32_t options;                /* 0 (MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED: tests only) */
  int32_t dim;                     /* 3 (default; 0 is read as 3) or 2; anything else is invalid */
  int32_t contrast_mode;           /* mad_pm_contrast_mode, MAD_PM_CONTRAST_ABSOLUTE (the word was
                                      reserved[0], which every earlier caller left 0) */
  union {
    int32_t channels;              /* C, 1..16 (0 is read as 1): planar vector-valued images with one
                                      joint diffusivity, "Vector-valued images" above.  The word is the
                                      first of the three reserved ones, which every earlier caller left
                                      0; `reserved` stays where it was and names it too */
    int32_t reserved[3];           /* [0] is channels; [1..2] stay 0 */
  };
} mad_pm_desc;

typedef struct mad_pm_stats {
  uint32_t iterations;             /* outer iterations run */
  uint32_t total_cycles;           /* MAD cycles over all iterations and steps */
  double last_relres;              /* relative residual at the end of the last step */
  double tensor_ms;                /* device time of the tensor generations, all iterations */
  double diffusion_ms;             /* MAD setup + solve, all iterations */
  double pass_ms[3];               /* device time per pass (z, y, x + map), summed over the
                                      iterations; dim 2: [0] is the fused kernel, [1..2] are 0.
                                      Quantile mode: the selection and the map kernel count with
                                      the last pass ([2], dim 2: [0]) */
  int32_t stalled;                 /* any step ended by the fp32 stall guard */
  int32_t tile[2];                 /* dim 2: the fused kernel's output tile (x, y); 0 in 3D */
  double contrast_used;            /* K of this run's last tensor generation: sqrt(s_q) in quantile mode (0
                                      when s_q = 0, and 0 for a run with iterations = 0, which has no
                                      generation), else the descriptor's contrast */
  int32_t reserved[2];
} mad_pm_stats;

/* the layout did not move: contrast_mode took reserved[0] of four, channels the next; contrast_used, behind 4 bytes of
 * padding, took the stats' reserved[0..2] */
#if defined(__cplusplus)
static_assert(sizeof(mad_pm_desc) == 176 && sizeof(mad_pm_stats) == 88, "mad_pm.h layout");
#else
_Static_assert(sizeof(mad_pm_desc) == 176 && sizeof(mad_pm_stats) == 88, "mad_pm.h layout");
#endif

typedef struct mad_pm_ctx mad_pm_ctx;

int mad_pm_desc_init(mad_pm_desc *d);
int mad_pm_create(const mad_pm_desc *d, mad_pm_ctx **out);
void mad_pm_destroy(mad_pm_ctx *ctx);
const char *mad_pm_last_error(const mad_pm_ctx *ctx);

/* The whole filter: host image in (any mad_dtype, x fastest), host image out (static_cast,
 * i.e. truncation for integer types).  MAD_ERR_NOT_CONVERGED (output written) when the stall
 * guard ended a diffusion step above the tolerance, as mad_ced_run.  Single GPU. */
int mad_pm_run(mad_pm_ctx *ctx, const void *in, int32_t in_dtype, void *out, int32_t out_dtype,
               mad_pm_stats *stats);
/* same with device buffers */
int mad_pm_run_device(mad_pm_ctx *ctx, const void *in, int32_t in_dtype, void *out,
                      int32_t out_dtype, mad_pm_stats *stats);

/* One tensor generation on a host image (parity / inspection).  tensor_soa: 6 arrays of N
 * doubles [xx,xy,xz,yy,yz,zz] (dim 2: 3 arrays [xx,xy,yy]); diffusivity (may be NULL): N
 * doubles, g itself. */
int mad_pm_tensor(mad_pm_ctx *ctx, const void *image, int32_t dtype, double *tensor_soa,
                  double *diffusivity);
/* Step 1 on a host image: dim arrays of N doubles, (gx, gy, gz) or (gx, gy). */
int mad_pm_gradient(mad_pm_ctx *ctx, const void *image, int32_t dtype, double *grad_soa);

#ifdef __cplusplus
}
#endif
#endif
