"""Perona-Malik contrast from a gradient quantile, fp64 numpy restatement -- TEST INFRASTRUCTURE
ONLY.  The package never imports this module.

Restates "Contrast from a quantile" of include/mad_pm.h on tests/pm_numpy.py (s and the map):

  rank   k = min(N - 1, max(0, ceil(q N) - 1)), product and ceil in fp64;
         s_q = the k-th smallest (0-based) s -- np.quantile(s, q, method="inverted_cdf")
  map    pm_numpy's step 3 with K^2 := s_q, used as it is (never via sqrt and squaring);
         the K reported is sqrt(s_q)
  s_q = 0: the limit K -> 0+ of all three diffusivities, g0 = 1 where s = 0, else 0
"""
import math

import numpy as np

import pm_numpy as P


def rank(q, n):
    """The 0-based rank of the quantile q among n values."""
    return min(n - 1, max(0, int(math.ceil(float(q) * float(n))) - 1))


def select(values, k):
    """The k-th smallest of the values (np.partition: exact, the value's own bits)."""
    a = np.asarray(values, np.float64).ravel()
    return float(np.partition(a, k)[k])


def quantile_s(s, q):
    """s_q."""
    return select(s, rank(q, np.asarray(s).size))


def diffusivity_k2(s, kind, k2, exponent=2.0, alpha=0.01):
    """pm_numpy.diffusivity with K^2 given directly; k2 = 0 takes the limit K -> 0+."""
    s = np.asarray(s, np.float64)
    if k2 == 0.0:
        g0 = np.where(s == 0.0, 1.0, 0.0)
    elif kind == P.WEICKERT:
        # pm_numpy's map squares its contrast: restate h(s) = exp(-(K^2 / s)^m) on K^2 itself
        with np.errstate(divide="ignore", over="ignore"):
            x = np.where(s > 0.0, k2 / np.where(s > 0.0, s, 1.0), np.inf)
            g0 = np.where(s > 0.0, 1.0 - np.exp(-(x ** exponent)), 1.0)
    elif kind == P.EXPONENTIAL:
        g0 = np.exp(-(s / k2))
    elif kind == P.RATIONAL:
        g0 = 1.0 / (1.0 + s / k2)
    else:
        raise ValueError("unknown diffusivity")
    return alpha + (1.0 - alpha) * g0


def pm_tensor(img, spacing, kind=P.WEICKERT, noise_scale=0.5, q=0.9, exponent=2.0, alpha=0.01):
    """(D, g, K) of quantile mode."""
    s = P.magnitude(P.gradient(img, spacing, noise_scale))
    k2 = quantile_s(s, q)
    g = diffusivity_k2(s, kind, k2, exponent, alpha)
    return P.tensor_from_diffusivity(g), g, math.sqrt(k2)


def pm_run(img, spacing, oracle_mod, q=0.9, **kw):
    """pm_numpy.pm_run with the contrast re-estimated from every iterate: (iterates, K per
    iteration)."""
    p = dict(P.DEFAULTS)
    p.update(kw)
    x = np.asarray(img, np.float64).copy()
    iterates, Ks = [], []
    for _ in range(p["iterations"]):
        T, _, K = pm_tensor(x, spacing, p["diffusivity"], p["noise_scale"], q, p["exponent"], p["alpha"])
        o = oracle_mod.Oracle(x.shape, spacing, T, p["time_step"])
        x = o.run(x, cycle=oracle_mod.VCYCLE, smoother=oracle_mod.GS_LEX,
                  iterations_per_grid=p["diffusion_iterations_per_grid"], max_cycles=100,
                  number_of_steps=p["diffusion_iterations"], tolerance=p["tolerance"])[0]
        iterates.append(x.copy())
        Ks.append(K)
    return iterates, Ks
