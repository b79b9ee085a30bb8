"""Structure-tensor diffusion tensors (Weickert's EED / CED), fp64 numpy restatement --
TEST INFRASTRUCTURE ONLY.  The package never imports this module.

Restates the definition of include/mad_ced.h (DESIGN.md "Structure-tensor diffusion") on
top of oracle/ved_oracle.py's taps and clamped correlation:

  1. g_d = K1(sigma) along d, K0(sigma) along the other two axes, passes z, y, x, then
     once * (1 / h_d)
  2. J0 = [gx gx, gx gy, gx gz, gy gy, gy gz, gz gz]
  3. J_rho = K0(rho) along x, then y, then z of each component (the clamp acts on J0)
  4. mu0 <= mu1 <= mu2, v_i = eigh(J_rho)   (LAPACK, independent of the GPU's Jacobi)
  5. h(d) = exp(-(K^2 / d)^m) for d > 0, else 0
       EED: lam_i = 1 - (1 - alpha) h(mu_i - mu0)
       CED: lam_i = alpha + (1 - alpha) h(mu2 - mu_i)
  6. D = sum lam_i v_i v_i^T, SoA [xx,xy,xz,yy,yz,zz]

Images are (z, y, x); spacing is (hx, hy, hz).
"""
import numpy as np

import ved_oracle as VO

EED, CED = 0, 1
DEFAULTS = dict(enhancement=EED, noise_scale=0.5, feature_scale=2.0, contrast=1.0, exponent=2.0,
                alpha=0.01, iterations=1, diffusion_iterations=5, time_step=0.1, tolerance=1e-6,
                diffusion_iterations_per_grid=2)
COMP = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def gradient(img, spacing, sigma):
    """(gx, gy, gz) at the noise scale."""
    img = np.asarray(img, np.float64)
    hx, hy, hz = spacing
    Kx, Ky, Kz = (VO.gauss_kernels(sigma, h) for h in (hx, hy, hz))
    z0, z1 = VO.correlate(img, Kz[0], 0), VO.correlate(img, Kz[1], 0)
    a00, a10, a01 = VO.correlate(z0, Ky[0], 1), VO.correlate(z0, Ky[1], 1), VO.correlate(z1, Ky[0], 1)
    gx = VO.correlate(a00, Kx[1], 2) * (1.0 / hx)
    gy = VO.correlate(a10, Kx[0], 2) * (1.0 / hy)
    gz = VO.correlate(a01, Kx[0], 2) * (1.0 / hz)
    return gx, gy, gz


def structure_tensor(img, spacing, sigma, rho):
    """J_rho, SoA (6, z, y, x)."""
    g = gradient(img, spacing, sigma)
    hx, hy, hz = spacing
    R = [VO.gauss_kernels(rho, h)[0] for h in (hx, hy, hz)]
    J = np.empty((6,) + g[0].shape)
    for c, (a, b) in enumerate(COMP):
        p = g[a] * g[b]
        p = VO.correlate(p, R[0], 2)
        p = VO.correlate(p, R[1], 1)
        J[c] = VO.correlate(p, R[2], 0)
    return J


def edge_stop(d, contrast, exponent):
    """h(d) = exp(-(K^2 / d)^m) for d > 0, 0 for d <= 0."""
    out = np.zeros_like(d)
    ok = d > 0
    with np.errstate(over="ignore", divide="ignore"):
        out[ok] = np.exp(-np.power(contrast * contrast / d[ok], exponent))
    return out


def eigenvalue_map(mu, enhancement, contrast, exponent, alpha):
    """lam (..., 3) from ascending mu (..., 3)."""
    if enhancement == EED:
        return 1.0 - (1.0 - alpha) * edge_stop(mu - mu[..., :1], contrast, exponent)
    if enhancement == CED:
        return alpha + (1.0 - alpha) * edge_stop(mu[..., 2:] - mu, contrast, exponent)
    raise ValueError("unknown enhancement")


def tensor_from_structure(J, enhancement=EED, contrast=1.0, exponent=2.0, alpha=0.01):
    """(D SoA (6, z, y, x), lam (3, z, y, x)) from J_rho SoA."""
    A = np.empty(J.shape[1:] + (3, 3))
    for c, (a, b) in enumerate(COMP):
        A[..., a, b] = J[c]
        A[..., b, a] = J[c]
    mu, V = np.linalg.eigh(A)
    lam = eigenvalue_map(mu, enhancement, contrast, exponent, alpha)
    T = np.einsum("...ik,...k,...jk->...ij", V, lam, V)
    D = np.stack([T[..., a, b] for a, b in COMP])
    return D, np.moveaxis(lam, -1, 0)


def ced_tensor(img, spacing, enhancement=EED, noise_scale=0.5, feature_scale=2.0, contrast=1.0,
               exponent=2.0, alpha=0.01):
    J = structure_tensor(img, spacing, noise_scale, feature_scale)
    return tensor_from_structure(J, enhancement, contrast, exponent, alpha)


def ced_run(img, spacing, oracle_mod, **kw):
    """The outer loop with the C MAD oracle for the diffusion steps: the list of iterates
    (one per outer iteration) and the per-iteration (cycles, relres)."""
    p = dict(DEFAULTS)
    p.update(kw)
    x = np.asarray(img, np.float64).copy()
    iterates, steps = [], []
    for _ in range(p["iterations"]):
        T, _ = ced_tensor(x, spacing, p["enhancement"], p["noise_scale"], p["feature_scale"],
                          p["contrast"], p["exponent"], p["alpha"])
        o = oracle_mod.Oracle(x.shape, spacing, T, p["time_step"])
        x, cyc, rr = o.run(x, cycle=p.get("cycle", oracle_mod.VCYCLE),
                           smoother=p.get("smoother", oracle_mod.GS_LEX),
                           iterations_per_grid=p["diffusion_iterations_per_grid"],
                           max_cycles=100, number_of_steps=p["diffusion_iterations"],
                           tolerance=p["tolerance"])
        iterates.append(x.copy())
        steps.append((cyc, rr))
    return iterates, steps
