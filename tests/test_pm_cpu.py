"""Regularised Perona-Malik diffusion (include/mad_pm.h) checks that need no GPU: the C ABI
surface, the descriptor defaults, the 2D kernel's tile plan, properties of the fp64 numpy
restatement (tests/pm_numpy.py) the GPU tests compare against, and parameter validation
(mad_pm_create validates before it touches a device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import pm_numpy as P
import synth
from conftest import ROOT
from multigridanisotropicdiffusion_amd import _capi as C

SP2, SP3 = (0.8, 1.25), (0.8, 1.0, 1.25)


def header_functions():
    src = open(os.path.join(ROOT, "include", "mad_pm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mad_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_pm_symbol():
    L = C.load()
    names = header_functions()
    assert len(names) == 8
    for n in names:
        assert hasattr(L, n), n


def test_pm_exports_equal_the_header_and_stand_apart():
    assert sorted(C.PM_EXPORTS) == header_functions()
    assert not set(C.PM_EXPORTS) & set(C.EXPORTS)
    assert not set(C.PM_EXPORTS) & set(C.CED_EXPORTS)


def test_desc_defaults():
    class Guarded(ctypes.Structure):
        _fields_ = [("d", C.PmDesc), ("guard", ctypes.c_uint8 * 16)]
    g = Guarded()
    ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
    assert C.load().mad_pm_desc_init(ctypes.byref(g.d)) == C.OK
    assert bytes(g.guard) == b"\xa5" * 16  # the library's struct is the binding's size
    d = g.d
    assert d.abi_version == C.ABI_VERSION
    assert d.diffusivity == C.PM_WEICKERT
    assert (C.PM_WEICKERT, C.PM_EXPONENTIAL, C.PM_RATIONAL) == (0, 1, 2)
    assert (d.noise_scale, d.contrast, d.exponent, d.alpha) == (0.5, 1.0, 2.0, 0.01)
    assert (d.iterations, d.diffusion_iterations) == (1, 5)
    assert d.cycle == C.VCYCLE and d.time_step == 0.1 and d.tolerance == 1e-6
    assert d.diffusion_iterations_per_grid == 2
    assert d.smoother == C.GAUSS_SEIDEL and d.precision == C.PRECISION_AUTO
    assert d.device == -1 and d.verbose == 0 and d.options == 0 and d.dim == 3
    assert list(d.size) == [1, 1, 1] and list(d.spacing) == [1.0, 1.0, 1.0]
    assert list(d.reserved) == [0, 0, 0, 0]
    assert len(C.PmStats().pass_ms) == 3 and len(C.PmStats().tile) == 2


def test_tile_plan():
    """The LDS arithmetic of the fused 2D kernel (pm_numpy.lds_bytes: max(image tile, gx | gy) +
    K0y u | K1y u), by hand for the rows the GPU test uses, spacing (0.8, 1.25):
      fp64 sigma 1     radii 5 / 4     64 x 32: (max(74 x 40, 2 x 32 x 65) + 2 x 74 x 33) x 8 = 72352 B,
                                       under 80 KiB: the full tile, two blocks per CU
      fp64 sigma 4     radii 20 / 13   64 x 32: (104 x 58 + 2 x 104 x 33) x 8 = 103168 B > 80 KiB,
                                       64 x 16: (104 x 42 + 2 x 104 x 17) x 8 = 63232 B: rows halved once
      fp64 sigma 14    radii 70 / 45   16 x 4: (156 x 94 + 2 x 156 x 5) x 8 = 129792 B <= 128 KiB: the floor
      fp64 sigma 14.25 radii 72 / 46   16 x 4: (160 x 96 + 2 x 160 x 5) x 8 = 135680 B: unsupported
    and the limits the header states for equal radii: 56 (fp64), 83 (fp32)."""
    assert P.radii(1.0, SP2) == (5, 4) and P.radii(1.0, SP3) == (5, 4, 4)
    assert P.lds_bytes(64, 32, 5, 4, 8) == (max(74 * 40, 2 * 32 * 65) + 2 * 74 * 33) * 8 == 72352
    assert P.tile_plan(5, 4, 8) == (64, 32, 72352)
    assert P.tile_plan(5, 4, 4) == (64, 32, 36176)
    assert P.radii(4.0, SP2) == (20, 13)
    assert P.lds_bytes(64, 32, 20, 13, 8) == (104 * 58 + 2 * 104 * 33) * 8 == 103168 > P.LDS_TWO_BLOCKS
    assert P.tile_plan(20, 13, 8) == (64, 16, (104 * 42 + 2 * 104 * 17) * 8) == (64, 16, 63232)
    assert P.radii(14.0, SP2) == (70, 45)
    assert P.tile_plan(70, 45, 8) == (16, 4, (156 * 94 + 2 * 156 * 5) * 8) == (16, 4, 129792)
    assert P.radii(14.25, SP2) == (72, 46)
    assert P.lds_bytes(16, 4, 72, 46, 8) == (160 * 96 + 2 * 160 * 5) * 8 == 135680 > P.LDS_CAP
    assert P.tile_plan(72, 46, 8) is None
    for sigma, tile in P.TILE_TABLE_FP64.items():
        plan = P.tile_plan(*P.radii(sigma, SP2), 8)
        assert (plan and plan[:2]) == tile, sigma
    # the header's limits
    assert P.tile_plan(56, 56, 8)[:2] == (16, 4) and P.tile_plan(57, 57, 8) is None
    assert P.tile_plan(83, 83, 4)[:2] == (16, 4) and P.tile_plan(84, 84, 4) is None
    # every plan keeps the kernel's preconditions: TW a power of two >= 16, TH a multiple of 4
    for R in range(1, 90):
        for elem in (4, 8):
            plan = P.tile_plan(R, max(1, R // 2), elem)
            if plan:
                assert plan[0] in (16, 32, 64) and plan[1] in (4, 8, 16, 32) and plan[2] <= P.LDS_CAP


@pytest.mark.parametrize("shape,sp", [((10, 11), SP2), ((9, 10, 11), SP3)])
@pytest.mark.parametrize("kind", [P.WEICKERT, P.EXPONENTIAL, P.RATIONAL])
def test_constant_image_gives_identity(shape, sp, kind):
    D, g = P.pm_tensor(np.full(shape, 37.5), sp, kind, 0.7, 5.0, 2.0, 0.01)
    assert np.abs(g - 1.0).max() < 1e-12
    diag = (0, 2) if len(shape) == 2 else (0, 3, 5)
    for c in range(D.shape[0]):
        assert np.abs(D[c] - (1.0 if c in diag else 0.0)).max() < 1e-12, c


@pytest.mark.parametrize("kind", [P.WEICKERT, P.EXPONENTIAL, P.RATIONAL])
def test_ramp_gives_the_analytic_diffusivity_in_the_interior(kind):
    """u = a x + b y in physical coordinates: the gradient is (a, b) wherever no tap is clamped,
    so g = g(a^2 + b^2) there."""
    shape, a, b, K, m, alpha = (30, 36), 3.0, -2.0, 3.5, 1.5, 0.02
    y, x = np.mgrid[:shape[0], :shape[1]]
    img = a * x * SP2[0] + b * y * SP2[1]
    _, g = P.pm_tensor(img, SP2, kind, 1.0, K, m, alpha)
    Rx, Ry = P.radii(1.0, SP2)
    s = a * a + b * b
    g0 = {P.WEICKERT: 1.0 - np.exp(-(K * K / s) ** m), P.EXPONENTIAL: np.exp(-s / (K * K)),
          P.RATIONAL: 1.0 / (1.0 + s / (K * K))}[kind]
    want = alpha + (1.0 - alpha) * g0
    assert 0.1 < want < 0.95
    assert np.abs(g[Ry:-Ry, Rx:-Rx] - want).max() < 1e-12


@pytest.mark.parametrize("kind", [P.WEICKERT, P.EXPONENTIAL, P.RATIONAL])
def test_diffusivity_is_monotone_and_lies_in_alpha_one(kind):
    alpha = 0.01
    s = np.concatenate([[0.0], np.logspace(-12, 12, 4001)])
    for m in (1.0, 1.5, 2.0, 3.0):
        g = P.diffusivity(s, kind, 5.0, m, alpha)
        assert g.min() >= alpha and g.max() <= 1.0
        assert np.all(np.diff(g) <= 0.0)
        assert g[0] == 1.0 and abs(g[-1] - alpha) < 1e-9


def test_weickert_diffusivity_is_eeds_across_edge_eigenvalue():
    """alpha + (1 - alpha)(1 - h) = 1 - (1 - alpha) h: the map EED applies to mu1 - mu0."""
    import ced2d_numpy as C2
    s = np.logspace(-3, 4, 200)
    mu = np.stack([np.zeros_like(s), s], axis=-1)
    lam = C2.eigenvalue_map(mu, C2.EED, 5.0, 2.0, 0.01)
    assert np.abs(lam[..., 1] - P.diffusivity(s, P.WEICKERT, 5.0, 2.0, 0.01)).max() < 1e-15


def test_monotonicity_measure():
    """pm_numpy.monotonicity on the behaviour tests' noisy step: the rational function at
    sigma = 1.5 stays under 1 (0.53), Weickert's at sigma = 0.7 is far over (21); a constant g
    gives 0 and a linear one its slope over twice its value."""
    assert P.monotonicity(np.full((5, 6), 0.3)) == 0.0
    g = np.broadcast_to(1.0 + 0.5 * np.arange(6.0), (5, 6))
    assert abs(P.monotonicity(g) - 1.0 / (4.0 * 1.5)) < 1e-15
    shape = (20, 24)
    x = np.arange(shape[1])
    img = np.where(x >= 12, 150.0, 100.0) + np.random.default_rng(3).normal(0.0, 2.0, size=shape)
    gentle = P.monotonicity(P.pm_tensor(img, (1.0, 1.0), P.RATIONAL, 1.5, 5.0, 2.0, 0.01)[1])
    sharp = P.monotonicity(P.pm_tensor(img, (1.0, 1.0), P.WEICKERT, 0.7, 5.0, 2.0, 0.01)[1])
    print(f"monotonicity: rational sigma 1.5 {gentle:.3f}, weickert sigma 0.7 {sharp:.2f}")
    assert gentle < 0.6 and sharp > 10.0


def test_fp32_emulation_is_fp32_and_close():
    """The emulation the GPU tests take their fp32 bounds from: fp32 throughout, within a few
    fp32 roundings of the fp64 restatement."""
    img = 100.0 * synth.image((9, 65), seed=9)
    g, g32 = P.gradient(img, SP2, 1.0), P.gradient_fp32(img, SP2, 1.0)
    scale = max(np.abs(c).max() for c in g)
    err = max(np.abs(a - b).max() for a, b in zip(g, g32)) / scale
    print(f"fp32 emulation: {err:.3e} of max|g|")
    assert 0.0 < err < 2e-6
    assert all(np.array_equal(c, c.astype(np.float32).astype(np.float64)) for c in g32)


def raw_create(**fields):
    """mad_pm_create on a descriptor filled by hand."""
    L = C.load()
    d = C.PmDesc()
    C.check(L.mad_pm_desc_init(ctypes.byref(d)))
    d.size[0], d.size[1], d.size[2] = fields.pop("size", (10, 9, 8))
    for k, val in fields.items():
        setattr(d, k, val)
    ctx = ctypes.c_void_p()
    rc = L.mad_pm_create(ctypes.byref(d), ctypes.byref(ctx))
    if rc != C.OK:
        raise C.MadError(rc, (L.mad_pm_last_error(None) or b"").decode())
    L.mad_pm_destroy(ctx)


@pytest.mark.parametrize("bad", [dict(noise_scale=0.0), dict(contrast=0.0), dict(contrast=-1.0),
                                 dict(exponent=0.0), dict(alpha=0.0), dict(alpha=1.0),
                                 dict(diffusivity=3), dict(diffusivity=-1), dict(options=1),
                                 dict(abi_version=C.ABI_VERSION + 1),
                                 dict(dim=2, size=(10, 9, 4)), dict(dim=1, size=(10, 1, 1)),
                                 dict(dim=4)])
def test_invalid_parameters(bad):
    with pytest.raises(C.MadError) as e:
        raw_create(**bad)
    assert e.value.code == C.ERR_INVALID
    assert len(str(e.value)) > len("mad error 1: ")


def test_python_context_rejects_bad_arguments():
    from multigridanisotropicdiffusion_amd import pm
    with pytest.raises(ValueError):
        pm.PM2D((8, 16, 16))
    with pytest.raises(ValueError):
        pm.PM((16, 16))
    with pytest.raises(ValueError):
        pm.PeronaMalikDiffusionImageFilter().SetDiffusivity("tukey")
    with pytest.raises(C.MadError) as e:
        pm.PM2D((9, 10), SP2, diffusivity=7)
    assert e.value.code == C.ERR_INVALID
