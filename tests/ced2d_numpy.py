"""2D structure-tensor diffusion tensors (EED / CED), fp64 numpy restatement -- TEST
INFRASTRUCTURE ONLY.  The package never imports this module.

Restates the 2D definition of include/mad_ced.h (DESIGN.md "Structure-tensor diffusion, 2D")
on oracle/ved_oracle.py's taps and clamped correlation, as tests/ced_numpy.py does in 3D:

  1. gx = K1x(K0y u) / hx, gy = K0x(K1y u) / hy   (pass along y, then x)
  2. J0 = [gx gx, gx gy, gy gy]
  3. J_rho = K0y(rho)(K0x(rho) J0)                 (x, then y; each clamp on the previous output)
  4. mu0 <= mu1, v_i = eigh(J_rho)                 (LAPACK, independent of the GPU's closed form)
  5. lam_i from ced_numpy.eigenvalue_map's rule on two eigenvalues
  6. D = sum lam_i v_i v_i^T, SoA [xx,xy,yy]

closed_form() is the tensor as the header writes it (no eigenvectors); the CPU test pins the
two against each other.  Images are (y, x); spacing is (hx, hy).
"""
import numpy as np

import ced_numpy as CN
import ved_oracle as VO

EED, CED = CN.EED, CN.CED
DEFAULTS = CN.DEFAULTS
COMP = ((0, 0), (0, 1), (1, 1))


def gradient(img, spacing, sigma):
    """(gx, gy) at the noise scale."""
    img = np.asarray(img, np.float64)
    hx, hy = spacing
    Kx, Ky = VO.gauss_kernels(sigma, hx), VO.gauss_kernels(sigma, hy)
    b0, b1 = VO.correlate(img, Ky[0], 0), VO.correlate(img, Ky[1], 0)
    gx = VO.correlate(b0, Kx[1], 1) * (1.0 / hx)
    gy = VO.correlate(b1, Kx[0], 1) * (1.0 / hy)
    return gx, gy


def structure_tensor(img, spacing, sigma, rho):
    """J_rho, SoA (3, y, x)."""
    g = gradient(img, spacing, sigma)
    Rx, Ry = VO.gauss_kernels(rho, spacing[0])[0], VO.gauss_kernels(rho, spacing[1])[0]
    J = np.empty((3,) + g[0].shape)
    for c, (a, b) in enumerate(COMP):
        J[c] = VO.correlate(VO.correlate(g[a] * g[b], Rx, 1), Ry, 0)
    return J


def eigenvalue_map(mu, enhancement, contrast, exponent, alpha):
    """lam (..., 2) from ascending mu (..., 2): the 3D rule on two eigenvalues."""
    if enhancement == EED:
        return 1.0 - (1.0 - alpha) * CN.edge_stop(mu - mu[..., :1], contrast, exponent)
    if enhancement == CED:
        return alpha + (1.0 - alpha) * CN.edge_stop(mu[..., 1:] - mu, contrast, exponent)
    raise ValueError("unknown enhancement")


def tensor_from_structure(J, enhancement=EED, contrast=1.0, exponent=2.0, alpha=0.01):
    """(D SoA (3, y, x), lam (2, y, x)) from J_rho SoA, through LAPACK's eigh."""
    A = np.empty(J.shape[1:] + (2, 2))
    for c, (a, b) in enumerate(COMP):
        A[..., a, b] = J[c]
        A[..., b, a] = J[c]
    mu, V = np.linalg.eigh(A)
    lam = eigenvalue_map(mu, enhancement, contrast, exponent, alpha)
    T = np.einsum("...ik,...k,...jk->...ij", V, lam, V)
    return np.stack([T[..., a, b] for a, b in COMP]), np.moveaxis(lam, -1, 0)


def closed_form(J, enhancement=EED, contrast=1.0, exponent=2.0, alpha=0.01):
    """(D, lam) as include/mad_ced.h writes steps 4-6 in 2D: r = hypot(d, b), the map on 2 r,
    D = s I + q [[d, b], [b, -d]]."""
    a, b, c = J
    d = 0.5 * (a - c)
    r = np.hypot(d, b)
    h = (1.0 - alpha) * CN.edge_stop(2.0 * r, contrast, exponent)
    if enhancement == EED:
        l0, l1 = np.ones_like(h), 1.0 - h
    else:
        l0, l1 = alpha + h, np.full_like(h, alpha)
    s = 0.5 * (l0 + l1)
    q = np.zeros_like(r)
    np.divide(l1 - l0, 2.0 * r, out=q, where=r > 0)
    return np.stack([s + q * d, q * b, s - q * d]), np.stack([l0, l1])


def ced_tensor(img, spacing, enhancement=EED, noise_scale=0.5, feature_scale=2.0, contrast=1.0,
               exponent=2.0, alpha=0.01):
    J = structure_tensor(img, spacing, noise_scale, feature_scale)
    return tensor_from_structure(J, enhancement, contrast, exponent, alpha)


def ced_run(img, spacing, oracle_mod, **kw):
    """The outer loop with the C MAD oracle (2D tensor [xx,xy,yy]) for the diffusion steps: the
    list of iterates (one per outer iteration) and the per-iteration (cycles, relres)."""
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
