"""2D structure-tensor diffusion on the GPU (include/mad_ced.h, dim = 2: the fused kernel
ced2_k) against the fp64 numpy restatement (tests/ced2d_numpy.py) and the C MAD oracle.

Every comparison prints its figure before asserting (pytest -s shows them).  The bounds:
  structure tensor: fp64 <= 1e-12 of max|J| (the kernel sums its taps in the restatement's
    order); fp32 <= TOL_J32 of max|J| = 4 x the largest error measured on an MI355X over SHAPES.
  tensor: fp64 <= TOL_D64, fp32 <= TOL_D32 absolute = 4 x measured, under the 3D test's
    ceilings 1e-6 / 1e-3.
  whole filter: fp64 <= 1e-8 of max|ref| against the restatement + oracle; fp32 <= 1e-5
    against the oracle run on the GPU's own tensor (the 3D filter bars).
"""
import ctypes
import os

import numpy as np
import pytest

import ced2d_numpy as C2
import synth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SP = (0.8, 1.25)
SIGMA, RHO = 0.7, 2.0  # radii 4 / 3 (sigma) and 10 / 7 (rho) along x / y
# (6, 7): every halo is longer than its axis (all indices clamped), one level; (9, 65): off the
# 64-lane width; (70, 300): crosses tile seams in both axes with the sigma + rho halo over each
# seam.  The tile is at most 64 columns x 32 rows, so no further shape is needed to cross it.
SHAPES = [(6, 7), (9, 65), (70, 300)]
TENSOR_SHAPES = [(6, 7), (9, 65), (26, 30)]
KW = dict(noise_scale=SIGMA, feature_scale=RHO, contrast=5.0, exponent=2.0, alpha=0.01)

# 4 x the largest error measured on an MI355X over the shapes above (each test's docstring
# lists the figures); the margin covers seed and shape variation
TOL_J32 = 4 * 3.19e-7   # of max|J|; the plain-numpy fp32 emulation gives 1.4e-7 ... 3.4e-7
TOL_D64 = 4 * 3.24e-15  # absolute; ceiling 1e-6
TOL_D32 = 4 * 2.29e-6   # absolute; ceiling 1e-3


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def image(shape):
    return 100.0 * synth.image(shape, seed=9)


_J = {}


def ref_structure(shape, rho=RHO):
    """J_rho of the restatement, computed once per (shape, rho) and left unchanged."""
    if (shape, rho) not in _J:
        J = C2.structure_tensor(image(shape), SP, SIGMA, rho)
        J.setflags(write=False)
        _J[(shape, rho)] = J
    return _J[(shape, rho)]


def relmax(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_structure_tensor_fp64(M, shape):
    """Measured on an MI355X: 3.3e-16, 3.6e-16, 2.8e-16 of max|J| for the three shapes."""
    v = M.CED2D(shape, SP, precision=M.FP64, **KW)
    J = v.structure_tensor(image(shape))
    v.close()
    assert J.shape == (3,) + shape
    err = relmax(J, ref_structure(shape))
    print(f"structure tensor 2D fp64 {shape}: {err:.3e} of max|J|")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_structure_tensor_fp32(M, shape):
    """fp32 storage and FIR arithmetic.  Measured on an MI355X: 3.18e-7, 2.92e-7, 3.08e-7 of max|J| for the
    three shapes (the plain-numpy fp32 emulation of steps 1-3 gives 1.4e-7 ... 3.4e-7); the
    bound is 4 x the largest."""
    v = M.CED2D(shape, SP, precision=M.FP32, **KW)
    J = v.structure_tensor(image(shape))
    v.close()
    err = relmax(J, ref_structure(shape))
    print(f"structure tensor 2D fp32 {shape}: {err:.3e} of max|J|")
    assert err <= TOL_J32


@pytest.mark.parametrize("enh", ["eed", "ced"])
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_tensor_matches_restatement(M, precision, enh):
    """K = 5 spreads lambda over [alpha, 1] (EED [0.0125, 1], CED [0.01, 0.9975] on (26, 30)).
    Measured max|D - ref| on an MI355X, shapes in TENSOR_SHAPES order:
      fp64 EED 1.7e-15, 1.7e-15, 2.9e-15;  fp64 CED 1.4e-15, 1.9e-15, 3.23e-15
      fp32 EED and CED alike 2.285e-6, 1.14e-6, 1.36e-6
    and max|lam - ref| 3.4e-15 (fp64), 2.35e-6 (fp32)
    (fp64: the closed form against LAPACK's eigh agrees to rounding; fp32: the fp32 J through
    the fp64 closed form).  Bounds: 4 x the largest of each precision."""
    tol = TOL_D64 if precision == "FP64" else TOL_D32
    assert tol <= (1e-6 if precision == "FP64" else 1e-3)
    worst = worst_l = 0.0
    for shape in TENSOR_SHAPES:
        v = M.CED2D(shape, SP, precision=getattr(M, precision), enhancement=enh, **KW)
        D, lam = v.tensor(image(shape), with_lambda=True)
        v.close()
        assert D.shape == (3,) + shape and lam.shape == (2,) + shape
        Dr, lr = C2.tensor_from_structure(ref_structure(shape), C2.EED if enh == "eed" else C2.CED,
                                          KW["contrast"], KW["exponent"], KW["alpha"])
        err, lerr = np.abs(D - Dr).max(), np.abs(lam - lr).max()
        print(f"tensor 2D {precision} {enh} {shape}: max|D - ref| = {err:.3e}, max|lam - ref| = {lerr:.3e}, "
              f"lam in [{lam.min():.4f}, {lam.max():.4f}]")
        worst, worst_l = max(worst, err), max(worst_l, lerr)
    # lam are the eigenvalues of D, and an eigenvalue of a symmetric 2 x 2 matrix moves by at most
    # the perturbation's 2-norm <= 2 max|entry| (Weyl)
    assert worst <= tol and worst_l <= 2 * tol


@pytest.mark.parametrize("exponent", [1.0, 1.5, 3.0])
def test_other_exponents(M, exponent):
    """The kernel takes (K^2 / t)^m without pow for m = 2 (every other test here) and m = 1; these
    run the other branches, fp64 on (26, 30), EED and CED.  Bound 1e-12 absolute, the bar that pins
    the closed form to eigh on the CPU: both sides work in fp64 on a J that agrees to 1e-15
    (measured <= 3.4e-15 for D, <= 3.6e-15 for lambda)."""
    shape = (26, 30)
    for enh in ("eed", "ced"):
        kw = dict(KW, exponent=exponent, enhancement=enh)
        v = M.CED2D(shape, SP, precision=M.FP64, **kw)
        D, lam = v.tensor(image(shape), with_lambda=True)
        v.close()
        Dr, lr = C2.tensor_from_structure(ref_structure(shape), C2.EED if enh == "eed" else C2.CED,
                                          kw["contrast"], exponent, kw["alpha"])
        err, lerr = np.abs(D - Dr).max(), np.abs(lam - lr).max()
        print(f"tensor 2D fp64 {enh} m = {exponent}: max|D - ref| = {err:.3e}, max|lam - ref| = {lerr:.3e}")
        assert err <= 1e-12 and lerr <= 1e-12


def test_reduced_tile(M):
    """fp64 storage, rho = 5: radii 25 / 16 along x / y.  The LDS arithmetic of ced2_generate (two
    regions, max(image tile, 3 products) + max(2 sigma-y arrays, 3 x-smoothed products), 8 B each):
    64 x 8 needs 185.8 KiB, 64 x 4 167.5 KiB, 32 x 4 121.7 KiB <= 128 KiB, so the host halves the rows
    to their floor and then the columns; at rho = 2 the tile is 64 x 8 (78.8 KiB).  (40, 90)
    crosses the reduced tile's seams in both axes with every halo longer than the tile.
    rho = 6 (radii 30 / 20) needs 137.9 KiB at the floor tile 16 x 4: unsupported."""
    shape = (40, 90)
    img = image(shape)
    tiles = {}
    for rho in (RHO, 5.0):
        v = M.CED2D(shape, SP, precision=M.FP64, diffusion_iterations=1, **dict(KW, feature_scale=rho))
        J = v.structure_tensor(img)
        _, st = v.run(img)
        v.close()
        tiles[rho] = st["tile"]
        err = relmax(J, ref_structure(shape, rho))
        print(f"reduced tile: rho {rho} tile {st['tile']}: {err:.3e} of max|J|")
        assert err <= 1e-12
    assert tiles[RHO] == (64, 8) and tiles[5.0] == (32, 4)
    v = M.CED2D(shape, SP, precision=M.FP64, **dict(KW, feature_scale=6.0))
    with pytest.raises(M.MadError) as e:
        v.structure_tensor(img)
    v.close()
    print(f"taps too long: {e.value}")
    assert e.value.code == M.capi.ERR_UNSUPPORTED
    assert len(str(e.value)) > len("mad error 6: ")


@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_constant_image_gives_identity(M, precision):
    shape = (10, 70)
    for enh, val in (("eed", 1.0), ("ced", 0.01)):
        v = M.CED2D(shape, SP, precision=getattr(M, precision), enhancement=enh, **KW)
        D = v.tensor(np.full(shape, 42.0))
        v.close()
        for c, want in enumerate((val, 0.0, val)):
            assert np.abs(D[c] - want).max() <= 1e-12, (enh, c)


def test_transposed_image_transposes_the_tensor(M):
    """Image (y, x) -> (x, y) with the spacing swapped: the phases run along the other axis with
    other radii, xx <-> yy.  fp64, <= 1e-9 (measured <= 2.9e-15)."""
    shape = (26, 30)
    img = image(shape)
    for enh in ("eed", "ced"):
        v = M.CED2D(shape, SP, precision=M.FP64, enhancement=enh, **KW)
        D = v.tensor(img)
        v.close()
        v = M.CED2D(shape[::-1], SP[::-1], precision=M.FP64, enhancement=enh, **KW)
        Dt = v.tensor(np.ascontiguousarray(img.T))
        v.close()
        for c, oc in enumerate((2, 1, 0)):
            err = np.abs(Dt[c] - D[oc].T).max()
            print(f"transpose 2D {enh} component {c}: {err:.3e}")
            assert err <= 1e-9, (enh, c)


FILTER_SHAPE = (26, 28)
FILTER_KW = dict(KW, enhancement="eed", diffusion_iterations=2, time_step=0.5, tolerance=1e-10)


def oracle_steps(oracle_mod, x, T, kw, spacing=SP):
    o = oracle_mod.Oracle(x.shape, spacing, T, kw["time_step"])
    return o.run(x, cycle=oracle_mod.VCYCLE, smoother=oracle_mod.GS_LEX, iterations_per_grid=2,
                 max_cycles=100, number_of_steps=kw["diffusion_iterations"], tolerance=kw["tolerance"])[0]


def test_filter_fp64_matches_restatement_and_oracle(M, oracle_mod):
    """Two outer iterations of two implicit steps, iteration by iteration, against the
    restatement's tensor fed to the C oracle: <= 1e-8 of max|ref| (measured 2.8e-10
    after iteration 1, 2.3e-10 after iteration 2; 8 and 16 cycles)."""
    img = image(FILTER_SHAPE)
    kw = dict(FILTER_KW, enhancement=C2.EED)
    refs, _ = C2.ced_run(img, SP, oracle_mod, iterations=2, **kw)
    for its in (1, 2):
        v = M.CED2D(FILTER_SHAPE, SP, precision=M.FP64, iterations=its, **FILTER_KW)
        out, st = v.run(img)
        v.close()
        err = relmax(out, refs[its - 1])
        print(f"filter 2D fp64 iteration {its}: {err:.3e} of max|ref|, cycles {st['total_cycles']}")
        assert st["iterations"] == its and st["total_cycles"] >= 2 * its
        assert err <= 1e-8


def test_filter_fp32_matches_oracle_on_its_own_tensor(M, oracle_mod):
    """fp32: each outer iteration's solve against the oracle run on the GPU's own tensor of
    that iteration's input: <= 1e-5 of max|ref| (measured 1.8e-7 and 2.1e-7)."""
    img = image(FILTER_SHAPE)
    v1 = M.CED2D(FILTER_SHAPE, SP, precision=M.FP32, iterations=1, **FILTER_KW)
    v2 = M.CED2D(FILTER_SHAPE, SP, precision=M.FP32, iterations=2, **FILTER_KW)
    out1, _ = v1.run(img)
    out2, st2 = v2.run(img)
    ref1 = oracle_steps(oracle_mod, img, v1.tensor(img), FILTER_KW)
    ref2 = oracle_steps(oracle_mod, out1, v1.tensor(out1), FILTER_KW)
    v1.close()
    v2.close()
    e1, e2 = relmax(out1, ref1), relmax(out2, ref2)
    print(f"filter 2D fp32: iteration 1 {e1:.3e}, iteration 2 {e2:.3e} of max|ref|")
    assert st2["iterations"] == 2
    assert e1 <= 1e-5 and e2 <= 1e-5


def test_lena(M, oracle_mod):
    """The reference's 2D test image (256 x 256), CED, unit spacing, 2 steps of 2.0: fp64 <= 1e-8
    of max|ref| against restatement + oracle, the default precision <= 1e-5 (measured
    7.4e-10 and 3.2e-6; 18 cycles against the oracle's 10 + 10)."""
    img = np.load(os.path.join(GOLDEN, "lena_256_u8.npy")).astype(np.float64)
    sp = (1.0, 1.0)
    kw = dict(noise_scale=SIGMA, feature_scale=RHO, contrast=5.0, exponent=2.0, alpha=0.01,
              diffusion_iterations=2, time_step=2.0, tolerance=1e-10)
    refs, steps = C2.ced_run(img, sp, oracle_mod, enhancement=C2.CED, **kw)
    for precision, tol in (("FP64", 1e-8), ("PRECISION_AUTO", 1e-5)):
        v = M.CED2D(img.shape, sp, enhancement="ced", precision=getattr(M, precision), **kw)
        out, st = v.run(img)
        v.close()
        err = relmax(out, refs[0])
        print(f"lena CED {precision}: {err:.3e} of max|ref|, cycles {st['total_cycles']} "
              f"(oracle {steps[0][0]}), tile {st['tile']}")
        assert err <= tol


@pytest.mark.parametrize("precision", ["PRECISION_AUTO", "FP64"])
def test_two_iterations_equal_two_chained_runs(M, precision):
    img = image(FILTER_SHAPE)
    kw = dict(FILTER_KW, tolerance=1e-6, precision=getattr(M, precision))
    v = M.CED2D(FILTER_SHAPE, SP, iterations=2, **kw)
    both, st = v.run(img)
    v.close()
    v = M.CED2D(FILTER_SHAPE, SP, iterations=1, **kw)
    a, sa = v.run(img)
    b, sb = v.run(a)
    v.close()
    assert st["total_cycles"] == sa["total_cycles"] + sb["total_cycles"]
    np.testing.assert_array_equal(both, b)


def test_eed_keeps_the_edge_and_smooths_the_flats(M):
    """A noisy step of 50 along x: EED (time step 2, 2 x 2 steps) keeps more of the jump than
    the identity tensor over the same 4 steps (with the oracle: 35.6 of 49.7 against 5.6), and
    the flat regions come out smoother than they went in (standard deviation 1.97 -> 0.18)."""
    shape = (20, 24)
    rng = np.random.default_rng(3)
    x = np.arange(shape[1])
    img = np.where(x >= 12, 150.0, 100.0) + rng.normal(0.0, 2.0, size=shape)
    v = M.CED2D(shape, (1.0, 1.0), enhancement="eed", noise_scale=0.7, feature_scale=2.0,
                contrast=5.0, alpha=0.01, time_step=2.0, iterations=2, diffusion_iterations=2)
    out, _ = v.run(img)
    v.close()
    s = M.Solver(shape, (1.0, 1.0), time_step=2.0, number_of_steps=4)
    I = np.zeros((3,) + shape)
    I[0] = I[2] = 1.0
    s.set_tensor(I)
    iso, _ = s.run(img, out_dtype=np.float64)
    s.close()
    jump = lambda u: float((u[:, 12] - u[:, 11]).mean())
    print(f"jump: input {jump(img):.2f}, EED {jump(out):.2f}, identity {jump(iso):.2f}")
    assert jump(out) > jump(iso)
    flat = lambda u: max(u[:, :8].std(), u[:, 16:].std())
    print(f"flat std: input {flat(img):.3f}, EED {flat(out):.3f}")
    assert flat(out) < flat(img)


def test_facade(M):
    shape = (14, 16)
    img = np.round(image(shape)).astype(np.int16)
    f = M.CoherenceEnhancingDiffusionImageFilter()
    f.SetInput(M.Image(img, spacing=SP, origin=(1.0, 2.0)))
    f.SetEnhancement("ced")
    f.SetNoiseScale(0.7)
    f.SetFeatureScale(1.5)
    f.SetContrast(5.0)
    f.SetAlpha(0.02)
    f.SetIterations(2)
    f.SetDiffusionIterations(2)
    f.SetTimeStep(0.2)
    out = f.Update()
    assert out is f.GetOutput()
    assert out.GetBufferAsArray().dtype == np.int16 and out.GetBufferAsArray().shape == shape
    assert out.spacing == SP and out.origin == (1.0, 2.0)
    assert f.stats["iterations"] == 2 and f.stats["total_cycles"] >= 4
    assert len(f.stats["pass_ms"]) == 5 and f.stats["pass_ms"][0] > 0.0
    assert f.stats["pass_ms"][1:] == [0.0] * 4 and f.stats["tensor_ms"] == f.stats["pass_ms"][0]
    # a 3D image through the same class still takes the 3D context
    vol = image((8, 9, 10)).astype(np.float32)
    f.SetInput(M.Image(vol, spacing=(0.8, 1.0, 1.25)))
    out = f.Update()
    assert out.GetBufferAsArray().dtype == np.float32 and out.GetBufferAsArray().shape == vol.shape
    assert f.stats["iterations"] == 2 and f.stats["tensor_ms"] > f.stats["pass_ms"][0] > 0.0


def raw_create(M, **fields):
    """mad_ced_create on a descriptor filled by hand; raises like CED2D does."""
    C = M.capi
    L = C.load()
    d = C.CedDesc()
    C.check(L.mad_ced_desc_init(ctypes.byref(d)))
    d.size[0], d.size[1], d.size[2] = fields.pop("size")
    for k, val in fields.items():
        setattr(d, k, val)
    ctx = ctypes.c_void_p()
    rc = L.mad_ced_create(ctypes.byref(d), ctypes.byref(ctx))
    if rc != C.OK:
        raise C.MadError(rc, (L.mad_ced_last_error(None) or b"").decode())
    L.mad_ced_destroy(ctx)


@pytest.mark.parametrize("fields", [dict(dim=2, size=(10, 9, 4)), dict(dim=1, size=(10, 1, 1)),
                                    dict(dim=4, size=(10, 9, 8))])
def test_invalid_dimension(M, fields):
    with pytest.raises(M.MadError) as e:
        raw_create(M, **fields)
    assert e.value.code == M.capi.ERR_INVALID
    assert len(str(e.value)) > len("mad error 1: ")


def test_dim_zero_is_read_as_three(M):
    """A caller built against the header without `dim` passes 0 there."""
    raw_create(M, dim=0, size=(10, 9, 8))


@pytest.mark.parametrize("bad", [dict(noise_scale=0.0), dict(feature_scale=-1.0), dict(contrast=0.0),
                                 dict(exponent=0.0), dict(alpha=0.0), dict(alpha=1.0),
                                 dict(enhancement=2)])
def test_invalid_parameters(M, bad):
    with pytest.raises(M.MadError) as e:
        M.CED2D((9, 10), SP, **bad)
    assert e.value.code == M.capi.ERR_INVALID
    assert len(str(e.value)) > len("mad error 1: ")


def test_three_dimensional_shape_raises(M):
    with pytest.raises(ValueError):
        M.CED2D((8, 16, 16))
