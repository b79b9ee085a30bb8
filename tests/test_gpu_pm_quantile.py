"""Perona-Malik contrast from a gradient quantile on the GPU (include/mad_pm.h "Contrast from a
quantile", include/mad_pm_quantile.h): the radix selection alone, the contrast, the
quantile-mode tensor and filter, against np.partition, the restatement
(tests/pm_quantile_numpy.py) and the C MAD oracle.

Every comparison prints its figure before asserting (pytest -s shows them).  The selection is
compared with == on the doubles everywhere.  Where a GPU contrast meets the restatement's, the
bound comes from the two s arrays at the neighbourhood of rank k.  With D = max|s(gpu) - s(ref)|
over the whole array, let delta be the same maximum over the voxels whose s(ref) lies within D
of s_q(ref).  Then |s_q(gpu) - s_q(ref)| <= delta: each of the at least k + 1 voxels with
s(ref) <= s_q(ref) has s(gpu) <= s_q(ref) + delta (inside the neighbourhood by delta's definition,
outside it because s(gpu) <= s(ref) + D < s_q(ref)), so the k-th smallest s(gpu) is at most
s_q(ref) + delta, and the mirror argument bounds it from below.  |sqrt a - sqrt b| / sqrt b <=
|a - b| / b then gives |K - K_ref| / K_ref <= delta / s_q(ref) (plus two roundings of the square roots).
"""
import math

import numpy as np
import pytest

import pm_numpy as P
import pm_quantile_numpy as Q
import synth

pytestmark = pytest.mark.gpu

SP2, SP3 = (0.8, 1.25), (0.8, 1.0, 1.25)
SIGMA = 1.0
KINDS = ["weickert", "exponential", "rational"]
QS = (0.5, 0.9, 1.0)
EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def ctx(M, shape, **kw):
    """PM2D or PM by the shape's dimension, at the seam tests' spacing and noise scale."""
    kw.setdefault("noise_scale", SIGMA)
    return (M.PM2D if len(shape) == 2 else M.PM)(shape, SP2 if len(shape) == 2 else SP3, **kw)


def image(shape):
    return 100.0 * synth.image(shape, seed=9)


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def own_s(v, img, precision):
    """s of the GPU's own gradient by step 2's rule: summed left to right in the storage
    precision (the gradient output holds the storage values exactly), then fp64."""
    G = v.gradient(img)
    return P.magnitude(G) if precision == "FP64" else P.magnitude_fp32(G)


# ------------------------------------------------------------------ 1. the selection alone

SIZES = [1, 2, 255, 256, 257, 4096 + 3, 2 ** 20 + 7]  # 2^20 + 7 also takes the candidate list


def contents(name, n, rng):
    if name == "uniform":
        return rng.random(n)
    if name == "all_equal":
        return np.full(n, 0.7)
    if name == "lowest_bit":
        return np.where(rng.random(n) < 0.5, 1.5, np.nextafter(1.5, 2.0))
    if name == "zeros_subnormals_huge":
        a = np.zeros(n)
        m = rng.random(n)
        sub = (m >= 0.90) & (m < 0.95)
        a[sub] = rng.integers(1, 2 ** 40, size=int(sub.sum())).astype(np.float64) * 5e-324
        big = m >= 0.95
        a[big] = np.finfo(np.float64).max / 4 * (1.0 - 0.5 * rng.random(int(big.sum())))
        return a
    if name == "sorted":
        return np.sort(rng.random(n) * 1e6)
    if name == "reverse_sorted":
        return np.sort(rng.random(n) * 1e-6)[::-1].copy()
    if name == "exact_floats":
        return (rng.random(n) * 1e4).astype(np.float32).astype(np.float64)
    raise ValueError(name)


@pytest.fixture(scope="module")
def selector(M):
    v = M.PM2D((8, 8))
    yield v
    v.close()


@pytest.mark.parametrize("name", ["uniform", "all_equal", "lowest_bit", "zeros_subnormals_huge", "sorted",
                                  "reverse_sorted", "exact_floats"])
def test_select_equals_partition(selector, name):
    """One lane, the edges of a wave and of a workgroup, a ragged last workgroup, many
    workgroups (and, from 65536 values, the candidate list); ranks 0, n // 2, n - 1."""
    rng = np.random.default_rng(11)
    for n in SIZES:
        a = contents(name, n, rng)
        assert a.min() >= 0.0 and np.isfinite(a).all()
        for k in sorted({0, n // 2, n - 1}):
            got, want = selector.select(a, k), Q.select(a, k)
            assert got == want and not (math.copysign(1.0, got) < 0), (name, n, k, got, want)


def test_select_repeats_and_leaves_nothing_behind(M, selector):
    """The same selection twice on one context, with another in between, and once on a fresh
    context: three identical results (scratch reuse leaves no stale counts or candidates)."""
    rng = np.random.default_rng(12)
    a = np.round(rng.random(2 ** 17 + 5) * 50.0) / 8.0  # ties; above the candidate-list threshold
    b = rng.random(70001) * 1e-3
    k = a.size // 3
    first = selector.select(a, k)
    assert selector.select(b, b.size - 1) == b.max()
    second = selector.select(a, k)
    other = M.PM((4, 5, 6))
    third = other.select(a, k)
    other.close()
    assert first == second == third == Q.select(a, k)
    assert selector.select(a[:300], 7) == Q.select(a[:300], 7)  # a short input after a long one


# ------------------------------------------------------------------ 2. the contrast

CONTRAST_SHAPES = [(6, 7), (9, 65), (70, 300), (5, 6, 7), (34, 35, 70)]
_REF_S = {}


def ref_s(shape):
    """The restatement's s, once per shape and left unchanged."""
    if shape not in _REF_S:
        s = P.magnitude(P.gradient(image(shape), SP2 if len(shape) == 2 else SP3, SIGMA))
        s.setflags(write=False)
        _REF_S[shape] = s
    return _REF_S[shape]


@pytest.mark.parametrize("shape", CONTRAST_SHAPES)
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_contrast(M, precision, shape):
    """mad_pm_contrast for q in {0.5, 0.9, 1.0} on the seam-crossing shapes.  Exact: K is the
    square root of the k-th smallest of the GPU's own s (from mad_pm_gradient's output by step
    2's rule).  Against the restatement: |K - K_ref| / K_ref <= delta / s_q(ref) + 2 eps with delta
    the measured max|s(gpu) - s(ref)| over the neighbourhood of rank k (module docstring).
    Measured on an MI355X, the largest |K - K_ref| / K_ref over the three q (its bound):
      fp64  (6, 7) 0 (4.4e-16), (9, 65) 7.1e-16 (1.7e-15), (70, 300) 0 (4.4e-16),
            (5, 6, 7) 3.8e-16 (1.3e-15), (34, 35, 70) 5.4e-16 (1.5e-15); 7 of the 15 are exactly 0
      fp32  (6, 7) 1.6e-7 (3.3e-7), (9, 65) 2.6e-7 (5.2e-7), (70, 300) 1.9e-7 (3.8e-7),
            (5, 6, 7) 2.8e-7 (5.7e-7), (34, 35, 70) 9.3e-8 (1.9e-7)
    The neighbourhood held one voxel, the one of rank k, in all 30 cases, and the bound is twice the
    fp32 error throughout (the square root halves a relative error); the whole-array maximum, which
    the test prints beside it, is up to 25 times looser."""
    img = image(shape)
    v = ctx(M, shape, precision=getattr(M, precision))
    s_gpu = own_s(v, img, precision)
    Ks = [v.contrast(img, q) for q in QS]
    v.close()
    s_ref = ref_s(shape)
    dist = np.abs(s_gpu - s_ref)
    D = dist.max()
    for q, K in zip(QS, Ks):
        k2 = Q.quantile_s(s_gpu, q)
        assert K == math.sqrt(k2), (q, K, math.sqrt(k2))
        k2_ref = Q.quantile_s(s_ref, q)
        K_ref = math.sqrt(k2_ref)
        near = np.abs(s_ref - k2_ref) <= D
        delta = dist[near].max()
        err, bound = abs(K - K_ref) / K_ref, delta / k2_ref + 2 * EPS
        print(f"contrast {precision} {shape} q = {q}: K = {K:.6f}, |K - K_ref| / K_ref = {err:.3e}, bound {bound:.3e} "
              f"({int(near.sum())} voxels near rank k; whole array: {D / k2_ref + 2 * EPS:.3e})")
        assert err <= bound
    assert Ks[0] < Ks[1] < Ks[2]
    assert D / np.abs(s_ref).max() <= (1e-12 if precision == "FP64" else 1e-5)


# ------------------------------------------------------------------ 3. the quantile-mode tensor

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_tensor_equals_absolute_mode_on_the_selected_k2(M, precision, kind):
    """Quantile mode's three phases (s, selection, map) give, bit for bit, what the fused
    absolute-mode kernel gives with K^2 forced to the same s_q (the test-only
    _contrast_squared: going through contrast = sqrt(s_q) would square-round)."""
    for shape in [(9, 65), (34, 35, 70)]:
        img = image(shape)
        kw = dict(precision=getattr(M, precision), diffusivity=kind, alpha=0.01)
        v = ctx(M, shape, contrast_quantile=0.9, **kw)
        D, g = v.tensor(img, with_diffusivity=True)
        D_only = v.tensor(img)
        k2 = Q.quantile_s(own_s(v, img, precision), 0.9)
        v.close()
        a = ctx(M, shape, _contrast_squared=k2, **kw)
        Da, ga = a.tensor(img, with_diffusivity=True)
        a.close()
        print(f"quantile tensor {precision} {kind} {shape}: K^2 = {k2:.6f}, g in [{g.min():.4f}, {g.max():.4f}]")
        assert g.min() < 0.5 < g.max()
        assert D.tobytes() == Da.tobytes() and g.tobytes() == ga.tobytes()
        assert D_only.tobytes() == D.tobytes()
        diag = (0, 2) if len(shape) == 2 else (0, 3, 5)
        for c in range(D.shape[0]):
            if c in diag:
                assert D[c].tobytes() == g.tobytes()
            else:
                assert not D[c].any() and not np.signbit(D[c]).any()
        # and the restatement's map on the same K^2
        gr = Q.diffusivity_k2(ref_s(shape), P.NAMES[kind], k2, 2.0, 0.01)
        assert np.abs(g - gr).max() <= (1e-12 if precision == "FP64" else 1e-3)


# ------------------------------------------------------------------ 4. scale covariance

@pytest.mark.parametrize("shape", [(70, 300), (34, 35, 70)])
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_scale_covariance(M, precision, shape):
    """u and 4 u: the tensors are the same bits and K scales by exactly 4 (a power of two
    scales every product of the passes exactly).  With a fixed contrast the pair differs."""
    u = image(shape)
    kw = dict(precision=getattr(M, precision), diffusion_iterations=1)
    v = ctx(M, shape, contrast_quantile=0.9, **kw)
    D1, D4 = v.tensor(u), v.tensor(4.0 * u)
    K1, K4 = v.contrast(u, 0.9), v.contrast(4.0 * u, 0.9)
    _, st1 = v.run(u)
    _, st4 = v.run(4.0 * u)
    v.close()
    print(f"scale covariance {precision} {shape}: K = {K1:.6f}, K(4 u) = {K4:.6f}")
    assert K1 > 0.0 and K4 == 4.0 * K1
    assert st1["contrast_used"] == K1 and st4["contrast_used"] == K4
    assert D1.tobytes() == D4.tobytes()
    assert D1[0].min() < 0.5 < D1[0].max()
    a = ctx(M, shape, contrast=K1, **kw)
    A1, A4 = a.tensor(u), a.tensor(4.0 * u)
    a.close()
    assert A1.tobytes() != A4.tobytes()
    assert np.abs(A1 - D1).max() <= 1e-6  # the same K up to the squaring: the mode itself changes nothing else


# ------------------------------------------------------------------ 5. degenerate: s_q = 0

@pytest.mark.parametrize("shape", [(20, 200), (6, 20, 200)])
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_zero_quantile(M, precision, shape):
    """q = 0.9.  A constant image and one whose left 95 % is constant select s_q = 0: K is
    reported as 0, the map takes the limit K -> 0+ (g = alpha + (1 - alpha) where s = 0, alpha
    elsewhere), nothing is NaN.  The constant is 0, for which every tap sum is exactly 0; for
    another constant c the derivative taps cancel only up to rounding and leave the same residue
    s ~ (eps c)^2 at every voxel, so K is 0 or that residue and g is one value everywhere
    (measured for c = 42: K = 1.0e-15 / 1.3e-15 in fp64 2D / 3D, 6.8e-7 / 7.6e-7 in fp32, and
    g = g(s = K^2): 0.636, 0.374, 0.505 for the three functions)."""
    alpha = 0.01
    one = alpha + (1.0 - alpha)
    rng = np.random.default_rng(4)
    edge = np.zeros(shape)
    edge[..., 190:] = 50.0 + 10.0 * rng.random(shape[:-1] + (10,))
    for kind in KINDS:
        v = ctx(M, shape, precision=getattr(M, precision), diffusivity=kind, alpha=alpha, contrast_quantile=0.9,
                diffusion_iterations=1)
        D, g = v.tensor(np.zeros(shape), with_diffusivity=True)
        assert v.contrast(np.zeros(shape), 0.9) == 0.0
        assert (g == one).all() and abs(one - 1.0) <= 2.3e-16 and not np.isnan(D).any()
        assert D.tobytes() == P.tensor_from_diffusivity(g).tobytes()
        D, g = v.tensor(edge, with_diffusivity=True)
        s = own_s(v, edge, precision)
        flat = (s == 0.0).mean()
        print(f"zero quantile {precision} {kind} {shape}: {flat:.1%} of the voxels flat")
        assert flat > 0.9 and v.contrast(edge, 0.9) == 0.0
        assert not np.isnan(D).any()
        assert g.tobytes() == np.where(s == 0.0, one, alpha).tobytes()
        out, st = v.run(edge)
        assert st["contrast_used"] == 0.0 and np.isfinite(out).all()
        D, g = v.tensor(np.full(shape, 42.0), with_diffusivity=True)
        K = v.contrast(np.full(shape, 42.0), 0.9)
        v.close()
        print(f"zero quantile {precision} {kind} {shape}: constant 42: K = {K:.3e}, g = {g.flat[0]:.6f}")
        assert 0.0 <= K <= 42.0 * (1e-12 if precision == "FP64" else 1e-4)
        assert len(np.unique(g)) == 1 and alpha <= g.flat[0] <= 1.0 and not np.isnan(D).any()


# ------------------------------------------------------------------ 6. the filter

FILTER_KW = dict(noise_scale=SIGMA, exponent=2.0, alpha=0.01, diffusion_iterations=2, time_step=0.5,
                 tolerance=1e-10)


@pytest.mark.parametrize("shape", [(26, 28), (12, 14, 16)])
def test_filter_reestimates_the_contrast_per_iteration(M, oracle_mod, shape):
    """Two outer iterations in quantile mode, fp64: equal to two chained one-iteration runs bit
    for bit; contrast_used is the second run's K (re-estimated from the iterate) and differs
    from the first's; the result matches the restatement + oracle at the fixed-contrast filter
    test's bar, <= 1e-8 of max|ref|.
    Measured on an MI355X: (26, 28) 2.1e-10 and 1.7e-10, K 13.466457 -> 5.887514, 17 cycles;
    (12, 14, 16) 1.7e-10 and 1.9e-10, K 9.306545 -> 3.574301, 21 cycles (the restatement prints
    the same K to all six digits)."""
    img = image(shape)
    sp = SP2 if len(shape) == 2 else SP3
    kw = dict(FILTER_KW, precision=M.FP64, contrast_quantile=0.9)
    v = ctx(M, shape, iterations=2, **kw)
    both, st = v.run(img)
    v.close()
    v = ctx(M, shape, iterations=1, **kw)
    a, sa = v.run(img)
    b, sb = v.run(a)
    v.close()
    np.testing.assert_array_equal(both, b)
    assert st["total_cycles"] == sa["total_cycles"] + sb["total_cycles"] and st["iterations"] == 2
    assert st["contrast_used"] == sb["contrast_used"] != sa["contrast_used"]
    assert sa["contrast_used"] > 0.0 and sb["contrast_used"] > 0.0
    kwr = {k: val for k, val in FILTER_KW.items()}
    refs, Ks = Q.pm_run(img, sp, oracle_mod, q=0.9, iterations=2, diffusivity=P.WEICKERT, **kwr)
    e1, e2 = relmax(a, refs[0]), relmax(both, refs[1])
    print(f"quantile filter {shape}: {e1:.3e}, {e2:.3e} of max|ref|; K {sa['contrast_used']:.6f} -> "
          f"{sb['contrast_used']:.6f} (restatement {Ks[0]:.6f} -> {Ks[1]:.6f}), cycles {st['total_cycles']}")
    assert e1 <= 1e-8 and e2 <= 1e-8


def test_facade(M):
    shape = (14, 16)
    img = image(shape)
    f = M.PeronaMalikDiffusionImageFilter(precision=M.FP64)
    f.SetInput(M.Image(img, spacing=SP2))
    f.SetNoiseScale(SIGMA)
    f.SetDiffusionIterations(1)
    f.SetContrastQuantile(0.9)
    assert f.GetContrastUsed() is None
    f.Update()
    K = f.GetContrastUsed()
    v = M.PM2D(shape, SP2, precision=M.FP64, noise_scale=SIGMA)
    assert K == v.contrast(img, 0.9) == f.stats["contrast_used"] and K > 0.0
    v.close()
    f.SetContrast(3.0)  # back to absolute mode
    f.Update()
    assert f.GetContrastUsed() == 3.0 and "contrast_used" not in f.stats


def test_run_without_a_generation_reports_no_contrast(M):
    """iterations = 0 is an identity run with no tensor generation: in quantile mode contrast_used
    is 0, on a fresh context (nothing of the selection is allocated yet) and after the inspection
    entry points have run on it (their result is not the run's); in absolute mode it is the
    descriptor's contrast, as in every run."""
    shape = (9, 10)
    img = image(shape)
    v = M.PM2D(shape, SP2, precision=M.FP64, iterations=0, contrast_quantile=0.9)
    assert v.contrast_used is None
    out, st = v.run(img)
    assert st["contrast_used"] == 0.0 and v.contrast_used == 0.0 and st["iterations"] == 0
    np.testing.assert_array_equal(out, img)
    assert v.contrast(img, 0.9) > 0.0 and v.select(np.arange(5.0) + 1.0, 2) == 3.0
    _, st = v.run(img)
    assert st["contrast_used"] == 0.0
    v.close()
    # a run's K is not overwritten by a later inspection call either
    v = M.PM2D(shape, SP2, precision=M.FP64, diffusion_iterations=1, contrast_quantile=0.9)
    _, st1 = v.run(img)
    assert v.select(np.arange(5.0) + 1.0, 2) == 3.0 and v.contrast(img, 0.5) < st1["contrast_used"]
    _, st2 = v.run(img)
    v.close()
    assert st2["contrast_used"] == st1["contrast_used"] > 0.0
    f = M.PeronaMalikDiffusionImageFilter(precision=M.FP64)
    f.SetInput(M.Image(img, spacing=SP2))
    f.SetContrastQuantile(0.9)
    f.SetNumberOfIterations(0)
    f.Update()
    assert f.GetContrastUsed() == 0.0
    a = M.PM2D(shape, SP2, iterations=0, contrast=2.5)
    a.run(img)
    assert a.contrast_used == 2.5
    a.close()


# ------------------------------------------------------------------ 7. validation

def test_validation(M):
    for bad in (dict(contrast_quantile=0.0), dict(contrast_quantile=1.0000001), dict(contrast_quantile=-0.1)):
        with pytest.raises(M.MadError) as e:
            M.PM2D((9, 10), SP2, **bad)
        assert e.value.code == M.capi.ERR_INVALID
    import ctypes
    C = M.capi
    d = C.PmDesc()
    C.check(C.load().mad_pm_desc_init(ctypes.byref(d)))
    d.contrast_mode = 2
    h = ctypes.c_void_p()
    assert C.load().mad_pm_create(ctypes.byref(d), ctypes.byref(h)) == C.ERR_INVALID and not h.value
    shape = (9, 10)
    img = image(shape)
    v = M.PM2D(shape, SP2, contrast=3.25, diffusion_iterations=1)
    a = np.arange(10.0)
    for n_k in ((10, 10), (10, -1)):
        with pytest.raises(M.MadError) as e:
            v.select(a[:n_k[0]], n_k[1])
        assert e.value.code == C.ERR_INVALID and "0 <= k < n" in str(e.value)
    with pytest.raises(M.MadError) as e:
        v.select(np.zeros(0), 0)
    assert e.value.code == C.ERR_INVALID
    for q in (0.0, 1.5):
        with pytest.raises(M.MadError) as e:
            v.contrast(img, q)
        assert e.value.code == C.ERR_INVALID
    assert v.select(a, 9) == 9.0  # the context is still usable
    # an absolute-mode context reports its own contrast and keeps its stats keys
    _, st = v.run(img)
    assert v.contrast_used == 3.25 and "contrast_used" not in st
    # mad_pm_contrast works in absolute mode too and leaves the mode alone
    K = v.contrast(img, 0.9)
    _, st = v.run(img)
    v.close()
    assert K > 0.0 and v.contrast_used == 3.25
