"""Structure-tensor diffusion on the GPU (include/mad_ced.h) against the fp64 numpy
restatement (tests/ced_numpy.py) and the C MAD oracle.

Every comparison prints its figure before asserting (pytest -s shows them).  The bounds:
  structure tensor: fp64 <= 1e-12 of max|J| (the FIR Hessian bar of the same machinery);
    fp32 <= TOL_J32 of max|J| = 4 x the largest error measured on an MI355X over SHAPES.
  tensor: fp64 <= TOL_D64, fp32 <= TOL_D32 absolute = 4 x measured, under the VED tensor
    ceilings 1e-6 / 1e-3.
  whole filter: fp64 <= 1e-8 of max|ref| against the restatement + oracle; fp32 <= 1e-5
    against the oracle run on the GPU's own tensor (the VED filter bars).
"""
import numpy as np
import pytest

import ced_numpy as CN
import synth

pytestmark = pytest.mark.gpu

SP = (0.8, 1.0, 1.25)
SIGMA, RHO = 0.7, 2.0
# (5, 6, 7): every halo is longer than its axis (all indices clamped); (33, 9, 65): off the
# 64-lane and 4-row blocks, two z tiles in fp32; (40, 70, 300): crosses a z tile, y tiles and
# the 256-wide x row with sigma + rho halos over each seam
SHAPES = [(5, 6, 7), (33, 9, 65), (40, 70, 300)]
TENSOR_SHAPES = [(5, 6, 7), (33, 9, 65), (22, 26, 30)]
KW = dict(noise_scale=SIGMA, feature_scale=RHO, contrast=5.0, exponent=2.0, alpha=0.01)

# 4 x the largest error measured on an MI355X over the shapes above (each test's docstring
# lists the figures); the margin covers seed and shape variation
TOL_J32 = 4 * 5.91e-7   # of max|J|; under 10 x the CPU fp32 emulation's 4.2e-7
TOL_D64 = 4 * 3.72e-15  # absolute; ceiling 1e-6
TOL_D32 = 4 * 1.15e-6   # absolute; ceiling 1e-3


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def image(shape):
    return 100.0 * synth.image(shape, seed=9)


_J = {}


def ref_structure(shape):
    """J_rho of the restatement, computed once per shape and left unchanged."""
    if shape not in _J:
        J = CN.structure_tensor(image(shape), SP, SIGMA, RHO)
        J.setflags(write=False)
        _J[shape] = J
    return _J[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_structure_tensor_fp64(M, shape):
    """Measured on an MI355X: 4.2e-16, 4.3e-16, 6.4e-16 of max|J| for the three shapes (the
    passes sum their taps in the restatement's order)."""
    v = M.CED(shape, SP, precision=M.FP64, **KW)
    J = v.structure_tensor(image(shape))
    v.close()
    ref = ref_structure(shape)
    err = np.abs(J - ref).max() / np.abs(ref).max()
    print(f"structure tensor fp64 {shape}: {err:.3e} of max|J|")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_structure_tensor_fp32(M, shape):
    """fp32 storage and FIR arithmetic.  Measured on an MI355X: 5.90e-7, 3.66e-7, 3.41e-7 of
    max|J| for the three shapes (the CPU fp32 emulation of steps 1-3 gives 4.2e-7 at
    (22, 26, 30)); the bound is 4 x the largest."""
    v = M.CED(shape, SP, precision=M.FP32, **KW)
    J = v.structure_tensor(image(shape))
    v.close()
    ref = ref_structure(shape)
    err = np.abs(J - ref).max() / np.abs(ref).max()
    print(f"structure tensor fp32 {shape}: {err:.3e} of max|J|")
    assert err <= TOL_J32


@pytest.mark.parametrize("enh", ["eed", "ced"])
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_tensor_matches_restatement(M, precision, enh):
    """K = 5 spreads lambda over the whole of [alpha, 1] (EED [0.016, 1], CED [0.01, 0.994] on
    these shapes).  Measured max|D - ref| on an MI355X, shapes in TENSOR_SHAPES order:
      fp64 EED 1.9e-15, 3.2e-15, 3.3e-15;  fp64 CED 2.2e-15, 3.6e-15, 3.7e-15
      fp32 EED 4.6e-7, 9.6e-7, 9.4e-7;     fp32 CED 8.1e-7, 1.14e-6, 9.4e-7
    (fp64: Jacobi rotations against LAPACK agree to rounding; fp32: the fp32 J through the
    fp64 eigen-analysis).  Bounds: 4 x the largest of each precision."""
    tol = TOL_D64 if precision == "FP64" else TOL_D32
    assert tol <= (1e-6 if precision == "FP64" else 1e-3)
    worst = 0.0
    for shape in TENSOR_SHAPES:
        v = M.CED(shape, SP, precision=getattr(M, precision), enhancement=enh, **KW)
        D, lam = v.tensor(image(shape), with_lambda=True)
        v.close()
        Dr, lr = CN.tensor_from_structure(ref_structure(shape), CN.EED if enh == "eed" else CN.CED,
                                          KW["contrast"], KW["exponent"], KW["alpha"])
        err, lerr = np.abs(D - Dr).max(), np.abs(lam - lr).max()
        print(f"tensor {precision} {enh} {shape}: max|D - ref| = {err:.3e}, max|lam - ref| = {lerr:.3e}, "
              f"lam in [{lam.min():.4f}, {lam.max():.4f}]")
        worst = max(worst, err)
    assert worst <= tol


@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_constant_volume_gives_identity(M, precision):
    shape = (9, 10, 70)
    for enh, val in (("eed", 1.0), ("ced", 0.01)):
        v = M.CED(shape, SP, precision=getattr(M, precision), enhancement=enh, **KW)
        D = v.tensor(np.full(shape, 42.0))
        v.close()
        for c, want in enumerate((val, 0.0, 0.0, val, 0.0, val)):
            assert np.abs(D[c] - want).max() <= 1e-12, (enh, c)


def test_transposed_image_transposes_the_tensor(M):
    """Image (z, y, x) -> (x, z, y), spacing permuted to match: the passes run along other
    axes with other tiles, the tensor components permute.  fp64, <= 1e-9 (measured <= 3.2e-15)."""
    shape = (22, 26, 30)
    img = image(shape)
    perm = (2, 0, 1)
    old = {0: 1, 1: 2, 2: 0}  # new physical axis -> old physical axis (0 = x)
    comp = {ab: c for c, ab in enumerate(CN.COMP)}
    for enh in ("eed", "ced"):
        v = M.CED(shape, SP, precision=M.FP64, enhancement=enh, **KW)
        D = v.tensor(img)
        v.close()
        imgp = np.ascontiguousarray(img.transpose(perm))
        v = M.CED(imgp.shape, (SP[1], SP[2], SP[0]), precision=M.FP64, enhancement=enh, **KW)
        Dp = v.tensor(imgp)
        v.close()
        for c, (a, b) in enumerate(CN.COMP):
            oc = comp[tuple(sorted((old[a], old[b])))]
            err = np.abs(Dp[c] - D[oc].transpose(perm)).max()
            print(f"transpose {enh} component {c}: {err:.3e}")
            assert err <= 1e-9, (enh, c)


FILTER_SHAPE = (24, 26, 28)
FILTER_KW = dict(KW, enhancement="eed", diffusion_iterations=2, time_step=0.5, tolerance=1e-10)


def relmax(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


def oracle_steps(oracle_mod, x, T, kw):
    o = oracle_mod.Oracle(x.shape, SP, T, kw["time_step"])
    return o.run(x, cycle=oracle_mod.VCYCLE, smoother=oracle_mod.GS_LEX, iterations_per_grid=2,
                 max_cycles=100, number_of_steps=kw["diffusion_iterations"], tolerance=kw["tolerance"])[0]


def test_filter_fp64_matches_restatement_and_oracle(M, oracle_mod):
    """Two outer iterations of two implicit steps, iteration by iteration, against the
    restatement's tensor fed to the C oracle: <= 1e-8 of max|ref| (measured 5.7e-11 after
    iteration 1, 4.8e-10 after iteration 2)."""
    img = image(FILTER_SHAPE)
    kw = dict(FILTER_KW, enhancement=CN.EED)
    refs, _ = CN.ced_run(img, SP, oracle_mod, iterations=2, **kw)
    for its in (1, 2):
        v = M.CED(FILTER_SHAPE, SP, precision=M.FP64, iterations=its, **FILTER_KW)
        out, st = v.run(img)
        v.close()
        err = relmax(out, refs[its - 1])
        print(f"filter fp64 iteration {its}: {err:.3e} of max|ref|, cycles {st['total_cycles']}")
        assert st["iterations"] == its and st["total_cycles"] >= 2 * its
        assert err <= 1e-8


def test_filter_fp32_matches_oracle_on_its_own_tensor(M, oracle_mod):
    """fp32: each outer iteration's solve against the oracle run on the GPU's own tensor of
    that iteration's input: <= 1e-5 of max|ref| (measured 2.7e-7 and 3.9e-7)."""
    img = image(FILTER_SHAPE)
    v1 = M.CED(FILTER_SHAPE, SP, precision=M.FP32, iterations=1, **FILTER_KW)
    v2 = M.CED(FILTER_SHAPE, SP, precision=M.FP32, iterations=2, **FILTER_KW)
    out1, _ = v1.run(img)
    out2, st2 = v2.run(img)
    ref1 = oracle_steps(oracle_mod, img, v1.tensor(img), FILTER_KW)
    ref2 = oracle_steps(oracle_mod, out1, v1.tensor(out1), FILTER_KW)
    v1.close()
    v2.close()
    e1, e2 = relmax(out1, ref1), relmax(out2, ref2)
    print(f"filter fp32: iteration 1 {e1:.3e}, iteration 2 {e2:.3e} of max|ref|")
    assert st2["iterations"] == 2
    assert e1 <= 1e-5 and e2 <= 1e-5


@pytest.mark.parametrize("precision", ["PRECISION_AUTO", "FP64"])
def test_two_iterations_equal_two_chained_runs(M, precision):
    img = image(FILTER_SHAPE)
    kw = dict(FILTER_KW, tolerance=1e-6, precision=getattr(M, precision))
    v = M.CED(FILTER_SHAPE, SP, iterations=2, **kw)
    both, st = v.run(img)
    v.close()
    v = M.CED(FILTER_SHAPE, SP, iterations=1, **kw)
    a, sa = v.run(img)
    b, sb = v.run(a)
    v.close()
    assert st["total_cycles"] == sa["total_cycles"] + sb["total_cycles"]
    np.testing.assert_array_equal(both, b)


def test_eed_keeps_the_edge_and_smooths_the_flats(M):
    """A noisy step of 50 along x: EED (time step 2, 2 x 2 steps) keeps more of the jump than
    the identity tensor over the same 4 steps (measured: 35.9 of 50 against 5.6), and the flat
    regions come out smoother than they went in (standard deviation 2.02 -> 0.07)."""
    shape = (16, 20, 24)
    rng = np.random.default_rng(3)
    x = np.arange(shape[2])
    img = np.where(x >= 12, 150.0, 100.0) + rng.normal(0.0, 2.0, size=shape)
    v = M.CED(shape, (1.0, 1.0, 1.0), enhancement="eed", noise_scale=0.7, feature_scale=2.0,
              contrast=5.0, alpha=0.01, time_step=2.0, iterations=2, diffusion_iterations=2)
    out, _ = v.run(img)
    v.close()
    s = M.Solver(shape, (1.0, 1.0, 1.0), time_step=2.0, number_of_steps=4)
    I = np.zeros((6,) + shape)
    I[0] = I[3] = I[5] = 1.0
    s.set_tensor(I)
    iso, _ = s.run(img, out_dtype=np.float64)
    s.close()
    jump = lambda u: float((u[:, :, 12] - u[:, :, 11]).mean())
    print(f"jump: input {jump(img):.2f}, EED {jump(out):.2f}, identity {jump(iso):.2f}")
    assert jump(out) > jump(iso)
    flat = lambda u: max(u[:, :, :8].std(), u[:, :, 16:].std())
    print(f"flat std: input {flat(img):.3f}, EED {flat(out):.3f}")
    assert flat(out) < flat(img)


def test_facade(M):
    shape = (12, 14, 16)
    img = np.round(image(shape)).astype(np.int16)
    f = M.CoherenceEnhancingDiffusionImageFilter()
    f.SetInput(M.Image(img, spacing=SP, origin=(1.0, 2.0, 3.0)))
    f.SetEnhancement("ced")
    f.SetNoiseScale(0.7)
    f.SetFeatureScale(1.5)
    f.SetContrast(5.0)
    f.SetExponent(2.0)
    f.SetAlpha(0.02)
    f.SetIterations(2)
    f.SetDiffusionIterations(2)
    f.SetTimeStep(0.2)
    f.SetTolerance(1e-6)
    f.SetCycle(f.VCYCLE)
    f.SetDiffusionIterationsPerGrid(2)
    out = f.Update()
    assert out is f.GetOutput()
    assert out.GetBufferAsArray().dtype == np.int16 and out.GetBufferAsArray().shape == shape
    assert out.spacing == SP and out.origin == (1.0, 2.0, 3.0)
    assert f.stats["iterations"] == 2 and f.stats["total_cycles"] >= 4
    assert len(f.stats["pass_ms"]) == 5 and f.stats["tensor_ms"] > 0.0


@pytest.mark.parametrize("bad", [dict(noise_scale=0.0), dict(feature_scale=-1.0), dict(contrast=0.0),
                                 dict(exponent=0.0), dict(alpha=0.0), dict(alpha=1.0),
                                 dict(enhancement=2)])
def test_invalid_parameters(M, bad):
    with pytest.raises(M.MadError) as e:
        M.CED((8, 9, 10), SP, **bad)
    assert e.value.code == M.capi.ERR_INVALID
    assert len(str(e.value)) > len("mad error 1: ")


def test_two_dimensional_shape_raises(M):
    with pytest.raises(ValueError):
        M.CED((16, 16))
