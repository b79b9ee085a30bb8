"""Regularised Perona-Malik diffusion tensors, fp64 numpy restatement -- TEST INFRASTRUCTURE
ONLY.  The package never imports this module.

Restates the definition of include/mad_pm.h (DESIGN.md "Nonlinear isotropic diffusion
(Perona-Malik)") on oracle/ved_oracle.py's taps and clamped correlation, in 2D and 3D:

  1. gradient at the noise scale: ced_numpy.gradient (3D, passes z, y, x) or
     ced2d_numpy.gradient (2D, y then x) -- the step 1 the structure-tensor filters share
  2. s = gx gx + gy gy (+ gz gz), summed left to right
  3. g0 = 1 - exp(-(K^2 / s)^m) for s > 0, else 1   (WEICKERT)
          exp(-s / K^2)                               (EXPONENTIAL)
          1 / (1 + s / K^2)                           (RATIONAL)
     g = alpha + (1 - alpha) g0
  4. D = g I, SoA [xx,xy,xz,yy,yz,zz] or [xx,xy,yy]

Images are (z, y, x) / (y, x); spacing is x first.  gradient_fp32 is a plain-numpy fp32
emulation of step 1 (multiply, then add, each rounded to fp32), from which the GPU tests take
their fp32 bounds; tile_plan restates the 2D kernel's host-side tile choice.
"""
import numpy as np

import ced2d_numpy as C2
import ced_numpy as CN
import ved_oracle as VO

WEICKERT, EXPONENTIAL, RATIONAL = 0, 1, 2
NAMES = {"weickert": WEICKERT, "exponential": EXPONENTIAL, "rational": RATIONAL}
DEFAULTS = dict(diffusivity=WEICKERT, noise_scale=0.5, contrast=1.0, exponent=2.0, alpha=0.01,
                iterations=1, diffusion_iterations=5, time_step=0.1, tolerance=1e-6,
                diffusion_iterations_per_grid=2)


def gradient(img, spacing, sigma):
    """(gx, gy) or (gx, gy, gz) at the noise scale, by the image's dimension."""
    img = np.asarray(img, np.float64)
    return (C2.gradient if img.ndim == 2 else CN.gradient)(img, spacing, sigma)


def magnitude(g):
    s = g[0] * g[0]
    for c in g[1:]:
        s = s + c * c
    return s


def diffusivity(s, kind=WEICKERT, contrast=1.0, exponent=2.0, alpha=0.01):
    """g(s), s the squared gradient magnitude."""
    s = np.asarray(s, np.float64)
    k2 = contrast * contrast
    if kind == WEICKERT:
        g0 = 1.0 - CN.edge_stop(s, contrast, exponent)
    elif kind == EXPONENTIAL:
        g0 = np.exp(-(s / k2))
    elif kind == RATIONAL:
        g0 = 1.0 / (1.0 + s / k2)
    else:
        raise ValueError("unknown diffusivity")
    return alpha + (1.0 - alpha) * g0


def tensor_from_diffusivity(g):
    """D = g I, SoA (3, y, x) or (6, z, y, x)."""
    ncomp = g.ndim * (g.ndim + 1) // 2
    D = np.zeros((ncomp,) + g.shape)
    for c in ((0, 2) if g.ndim == 2 else (0, 3, 5)):
        D[c] = g
    return D


def pm_tensor(img, spacing, diffusivity_kind=WEICKERT, noise_scale=0.5, contrast=1.0, exponent=2.0,
              alpha=0.01):
    """(D, g)."""
    g = diffusivity(magnitude(gradient(img, spacing, noise_scale)), diffusivity_kind, contrast,
                    exponent, alpha)
    return tensor_from_diffusivity(g), g


def pm_run(img, spacing, oracle_mod, **kw):
    """The outer loop with the C MAD oracle for the diffusion steps: the list of iterates (one
    per outer iteration) and the per-iteration (cycles, relres)."""
    p = dict(DEFAULTS)
    p.update(kw)
    x = np.asarray(img, np.float64).copy()
    iterates, steps = [], []
    for _ in range(p["iterations"]):
        T, _ = pm_tensor(x, spacing, p["diffusivity"], p["noise_scale"], p["contrast"], p["exponent"],
                         p["alpha"])
        o = oracle_mod.Oracle(x.shape, spacing, T, p["time_step"])
        x, cyc, rr = o.run(x, cycle=p.get("cycle", oracle_mod.VCYCLE),
                           smoother=p.get("smoother", oracle_mod.GS_LEX),
                           iterations_per_grid=p["diffusion_iterations_per_grid"],
                           max_cycles=100, number_of_steps=p["diffusion_iterations"],
                           tolerance=p["tolerance"])
        iterates.append(x.copy())
        steps.append((cyc, rr))
    return iterates, steps


# ---------------------------------------------------------------- fp32 emulation of step 1

def _correlate32(f, K, axis):
    """ved_oracle.correlate with every product and every sum rounded to fp32."""
    K = np.asarray(K, np.float32)
    R = (len(K) - 1) // 2
    n = f.shape[axis]
    out = np.zeros_like(f)
    for q, t in enumerate(range(-R, R + 1)):
        idx = np.clip(np.arange(n) + t, 0, n - 1)
        out = out + K[q] * np.take(f, idx, axis=axis)
    assert out.dtype == np.float32
    return out


def gradient_fp32(img, spacing, sigma):
    """Step 1 in fp32 storage and arithmetic (taps and 1 / h rounded to fp32, multiply then add),
    returned as fp64 arrays.  Independent of the GPU code: no fma, numpy's own loop order."""
    u = np.asarray(img, np.float64).astype(np.float32)
    K = [VO.gauss_kernels(sigma, h) for h in spacing]
    ih = [np.float32(1.0 / h) for h in spacing]
    if u.ndim == 2:
        b0, b1 = _correlate32(u, K[1][0], 0), _correlate32(u, K[1][1], 0)
        g = (_correlate32(b0, K[0][1], 1) * ih[0], _correlate32(b1, K[0][0], 1) * ih[1])
    else:
        z0, z1 = _correlate32(u, K[2][0], 0), _correlate32(u, K[2][1], 0)
        a00, a10, a01 = _correlate32(z0, K[1][0], 1), _correlate32(z0, K[1][1], 1), _correlate32(z1, K[1][0], 1)
        g = (_correlate32(a00, K[0][1], 2) * ih[0], _correlate32(a10, K[0][0], 2) * ih[1],
             _correlate32(a01, K[0][0], 2) * ih[2])
    assert all(c.dtype == np.float32 for c in g)
    return tuple(c.astype(np.float64) for c in g)


def magnitude_fp32(g):
    """s of an fp32 gradient (given as fp64 arrays holding fp32 values), summed in fp32."""
    g = [c.astype(np.float32) for c in g]
    s = g[0] * g[0]
    for c in g[1:]:
        s = s + c * c
    return s.astype(np.float64)


# ---------------------------------------------------------------- the 2D kernel's tile plan

LDS_CAP = 128 * 1024       # the dynamic LDS cap of the FIR tiles
LDS_TWO_BLOCKS = 80 * 1024  # half a CU's 160 KiB


def lds_bytes(TW, TH, Rx, Ry, elem):
    """LDS of the fused 2D kernel for a TW x TH tile: region 1 = max(image tile, gx | gy with row
    pitch TW + 1), region 2 = K0y u | K1y u, column-major with pitch TH + 1."""
    WA, HA = TW + 2 * Rx, TH + 2 * Ry
    return (max(WA * HA, 2 * TH * (TW + 1)) + 2 * WA * (TH + 1)) * elem


def tile_plan(Rx, Ry, elem):
    """(TW, TH, bytes), or None when the taps do not fit the smallest tile: start at 64 x 32,
    halve the rows down to 8 while the block is over half a CU's LDS, then rows (to 4) before
    columns (to 16) while it is over the cap."""
    TW, TH = 64, 32
    b = lambda: lds_bytes(TW, TH, Rx, Ry, elem)
    while TH > 8 and b() > LDS_TWO_BLOCKS:
        TH //= 2
    while TH > 4 and b() > LDS_CAP:
        TH //= 2
    while TW > 16 and b() > LDS_CAP:
        TW //= 2
    return (TW, TH, b()) if b() <= LDS_CAP else None


def radii(sigma, spacing):
    return tuple(VO.kernel_radius(sigma, h) for h in spacing)


# the fused kernel's tile in MAD_FP64 at spacing (0.8, 1.25) by sigma (None: taps too long);
# tests/test_pm_cpu.py::test_tile_plan proves each row from the LDS arithmetic
TILE_TABLE_FP64 = {1.0: (64, 32), 4.0: (64, 16), 14.0: (16, 4), 14.25: None}


def row_contrast(s):
    """The contrast a parity test uses for an image with squared gradient magnitudes s: the
    median gradient magnitude, so g spreads over both sides of the map's slope."""
    return float(np.sqrt(np.median(s)))


def monotonicity(g):
    """max |g(p + 1) - g(p - 1)| / (4 g(p)) over the axes and the interior points.  The MAD
    stencil (the reference's, oracle/mad_oracle.c generate_dca) discretises div(g grad u) as
    g lap u + grad g . grad u with central differences: the neighbour weights along an axis are
    -dt / h^2 (g(p) +- (g(p + 1) - g(p - 1)) / 4), so up to 1 every off-diagonal weight is
    non-positive (an M-matrix: no over- or undershoot at any time step); above 1 the implicit
    step can leave the input's range."""
    worst = 0.0
    for ax in range(g.ndim):
        lo, mid, hi = (np.take(g, range(a, g.shape[ax] - 2 + a), axis=ax) for a in (0, 1, 2))
        worst = max(worst, float((np.abs(hi - lo) / (4.0 * mid)).max()))
    return worst
