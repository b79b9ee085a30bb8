/*
 * mad_ced.h -- C ABI of the structure-tensor diffusion filters on the GPU: Weickert's
 * edge-enhancing (EED) and coherence-enhancing (CED) diffusion, a sibling of the VED
 * pipeline of mad_ved.h.  The diffusion tensor is derived from the image's smoothed
 * structure tensor on the device and handed to the MAD solver of mad.h in place.
 *
 * Definition (3D, image u, spacing h, borders replicated by index clamping, x fastest;
 * K0 / K1 the sampled Gaussian / first-derivative taps of mad_ved.h's FIR operator,
 * radius max(1, ceil(4 s / h_d)) for a physical scale s on axis d):
 *   1. gradient at the noise scale sigma: g_d = K1(sigma) along d, K0(sigma) along the
 *      other two axes (passes z, y, x; correlation sum_t K(t) f(clamp(i + t))), times 1 / h_d
 *   2. products J0 = [gx gx, gx gy, gx gz, gy gy, gy gz, gz gz]
 *   3. integration at the feature scale rho: K0(rho) along x, y, z of each component
 *      (the clamp acts on J0)
 *   4. eigen-analysis of J_rho: mu0 <= mu1 <= mu2, orthonormal v_i
 *   5. with h(d) = exp(-(K^2 / d)^m) for d > 0 and 0 otherwise (contrast K, exponent m):
 *        EED: lambda_i = 1 - (1 - alpha) h(mu_i - mu0)
 *        CED: lambda_i = alpha + (1 - alpha) h(mu2 - mu_i)
 *   6. D = sum_i lambda_i v_i v_i^T, fp64 SoA [xx,xy,xz,yy,yz,zz]
 * Outer loop as in VED: per iteration one tensor generation from the current image, then
 * diffusion_iterations implicit steps of time_step through the MAD solver.
 * See DESIGN.md "Structure-tensor diffusion" and tests/ced_numpy.py.
 *
 * Limit on the scales (3D): every pass keeps its tile and the taps' halo in 128 KiB of LDS and
 * shrinks the tile for long taps; taps that do not fit the smallest tile make
 * mad_ced_run, mad_ced_tensor and mad_ced_structure_tensor return MAD_ERR_UNSUPPORTED
 * ("Gaussian taps too long for the LDS tiles") before anything is launched; the context stays
 * usable and is destroyed as usual.  The last pass sets the limit: it holds 4 + 2 R planes of
 * six volumes over 64 columns, R = max(1, ceil(4 rho / h_z)) the radius of the feature scale
 * along z, which fits for R <= 19 in MAD_FP64 (rho <= 4.75 h_z) and R <= 40 with fp32 storage
 * (rho <= 10 h_z).  fp32 storage, the default precision, is the way past the fp64 limit.  The
 * other passes allow more (fp64 / fp32 radii: sigma along z 30 / 62, sigma along y 62 / 126,
 * rho along y 126 / 254).  2D has its own limit, DESIGN.md "Structure-tensor diffusion, 2D".
 *
 * 2D (mad_ced_desc.dim == 2, image u(y, x), spacing (hx, hy), size[2] == 1): the same
 * definition minus the z axis, computed by one fused kernel per tensor generation.
 *   1. gx = K1x(K0y u) / hx, gy = K0x(K1y u) / hy (pass along y first, then x)
 *   2. J0 = [gx gx, gx gy, gy gy]
 *   3. J_rho = K0y(rho)(K0x(rho) J0): x first, then y; the x clamp acts on J0, the y clamp
 *      on the x-smoothed products
 *   4. with J_rho = [[a, b], [b, c]]: m = (a + c) / 2, d = (a - c) / 2, r = hypot(d, b),
 *      mu0 = m - r, mu1 = m + r; mu1 - mu0 is taken as 2 r, never as a difference
 *   5. EED: lambda0 = 1, lambda1 = 1 - (1 - alpha) h(2 r)
 *      CED: lambda0 = alpha + (1 - alpha) h(2 r), lambda1 = alpha
 *   6. D = s I + q [[d, b], [b, -d]], s = (lambda0 + lambda1) / 2,
 *      q = (lambda1 - lambda0) / (2 r) for r > 0, else 0 (= sum_i lambda_i v_i v_i^T without
 *      eigenvectors, continuous at r = 0); fp64 SoA [xx,xy,yy]
 * Steps 4-6 run in fp64 in every precision mode.  mad_ced_tensor then writes 3 arrays
 * [xx,xy,yy] and 2 lambda arrays (lambda0, lambda1: the order of the ascending mu),
 * mad_ced_structure_tensor 3 arrays; mad_ced_run / mad_ced_run_device behave as in 3D.
 * mad_ced_stats.pass_ms[0] carries the fused kernel's time, entries 1-4 are 0.
 * See DESIGN.md "Structure-tensor diffusion, 2D" and tests/ced2d_numpy.py.
 */
#ifndef MAD_CED_H
#define MAD_CED_H

#include "mad.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum mad_ced_enhancement {
  MAD_CED_EED = 0,                 /* edge enhancing: smooths along edges, not across */
  MAD_CED_CED = 1                  /* coherence enhancing: smooths along the coherence direction */
} mad_ced_enhancement;

typedef struct mad_ced_desc {
  uint32_t abi_version;            /* MAD_ABI_VERSION */
  int64_t size[3];                 /* x, y, z (dim 2: z = 1) */
  double spacing[3];               /* image spacing, x first (dim 2: spacing[2] is ignored) */
  int32_t enhancement;             /* mad_ced_enhancement, MAD_CED_EED */
  double noise_scale;              /* sigma, physical units, 0.5 */
  double feature_scale;            /* rho, physical units, 2.0 */
  double contrast;                 /* K, 1.0 */
  double exponent;                 /* m, 2.0 */
  double alpha;                    /* 0 < alpha < 1, 0.01 */
  uint32_t iterations;             /* 1  (outer iterations: tensor generation + diffusion) */
  uint32_t diffusion_iterations;   /* 5  (MAD NumberOfSteps per iteration) */
  /* MAD parameters of the diffusion steps (MaxCycles fixed at 100, as in VED) */
  int32_t cycle;                   /* MAD_VCYCLE */
  double time_step;                /* 0.1 */
  double tolerance;                /* 1e-6 */
  uint32_t diffusion_iterations_per_grid; /* 2 */
  int32_t smoother;                /* mad_smoother, MAD_GAUSS_SEIDEL */
  int32_t precision;               /* MAD_PRECISION_AUTO (default) / MAD_FP32 / MAD_FP32_REFINE: fp32
                                      passes, the diffusion solve as mad_create resolves it;
                                      MAD_FP64: fp64 throughout.  The eigen-analysis and the
                                      eigenvalue map run in fp64 in every mode. */
  int32_t device;                  /* HIP device, -1 = current */
  int32_t verbose;                 /* 0 */
  uint32_t options;                /* reserved, 0 */
  int32_t dim;                     /* 3 (default; 0 is read as 3, the value a caller built before
                                      this field existed passes) or 2; anything else is invalid */
  int32_t reserved[4];
} mad_ced_desc;

typedef struct mad_ced_stats {
  uint32_t iterations;             /* outer iterations run */
  uint32_t total_cycles;           /* MAD cycles over all iterations and steps */
  double last_relres;              /* relative residual at the end of the last step */
  double tensor_ms;                /* device time of the tensor generations, all iterations */
  double diffusion_ms;             /* MAD setup + solve, all iterations */
  double pass_ms[5];               /* device time per pass (z, y, x + products, rho y, rho z +
                                      eigen), summed over the iterations; dim 2: [0] is the fused
                                      kernel, [1..4] are 0 */
  int32_t stalled;                 /* any step ended by the fp32 stall guard */
  int32_t tile[2];                 /* dim 2: the fused kernel's output tile (x, y); 0 in 3D */
  int32_t reserved[5];
} mad_ced_stats;

typedef struct mad_ced_ctx mad_ced_ctx;

int mad_ced_desc_init(mad_ced_desc *d);
int mad_ced_create(const mad_ced_desc *d, mad_ced_ctx **out);
void mad_ced_destroy(mad_ced_ctx *ctx);
const char *mad_ced_last_error(const mad_ced_ctx *ctx);

/* The whole filter: host image in (any mad_dtype, x fastest), host image out (static_cast,
 * i.e. truncation for integer types).  MAD_ERR_NOT_CONVERGED (output written) when the stall
 * guard ended a diffusion step above the tolerance, as mad_ved_run.  Single GPU. */
int mad_ced_run(mad_ced_ctx *ctx, const void *in, int32_t in_dtype, void *out,
                int32_t out_dtype, mad_ced_stats *stats);
/* same with device buffers */
int mad_ced_run_device(mad_ced_ctx *ctx, const void *in, int32_t in_dtype, void *out,
                       int32_t out_dtype, mad_ced_stats *stats);

/* One tensor generation on a host image (parity / inspection).  tensor_soa: 6 arrays of N
 * doubles [xx,xy,xz,yy,yz,zz]; lambda_soa (may be NULL): 3 arrays of N doubles, the mapped
 * eigenvalues in the order of the ascending structure-tensor eigenvalues.  dim 2: 3 arrays
 * [xx,xy,yy] and 2 lambda arrays. */
int mad_ced_tensor(mad_ced_ctx *ctx, const void *image, int32_t dtype, double *tensor_soa,
                   double *lambda_soa);
/* Steps 1-3 on a host image: J_rho, 6 arrays of N doubles (dim 2: 3 arrays). */
int mad_ced_structure_tensor(mad_ced_ctx *ctx, const void *image, int32_t dtype,
                             double *structure_soa);

#ifdef __cplusplus
}
#endif
#endif
