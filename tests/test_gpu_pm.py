"""3D regularised Perona-Malik diffusion on the GPU (include/mad_pm.h: the gradient passes
ced_z_k and ced_y_k, then pm_x_k) against the fp64 numpy restatement (tests/pm_numpy.py) and the
C MAD oracle.

Every comparison prints its figure before asserting (pytest -s shows them).  The bounds are
those of tests/test_gpu_pm2d.py:
  gradient: fp64 <= 1e-12 of max|g|; fp32 <= 4 x the error of the plain-numpy fp32 emulation of
    step 1 (pm_numpy.gradient_fp32) against the fp64 restatement.
  tensor / diffusivity: fp64 <= 1e-12 absolute; fp32 <= 4 x the error of the emulated fp32
    gradient pushed through the fp64 map, and under the project's ceiling 1e-3.
  whole filter: fp64 <= 1e-8 of max|ref| against the restatement + oracle; fp32 <= 1e-5 against
    the oracle run on the GPU's own tensor.
"""
import numpy as np
import pytest

import pm_numpy as P
import synth

pytestmark = pytest.mark.gpu

SP = (0.8, 1.0, 1.25)
SIGMA = 1.0  # radii 5 / 4 / 4 along x / y / z
# (3, 4, 5): every halo is at least its axis; (34, 35, 70): crosses the 32-plane z tile, the
# 32-row y tile and the 64-column blocks; (3, 5, 260): the 256-wide x row with a 4-wide last
# block narrower than the x radius.
SHAPES = [(3, 4, 5), (34, 35, 70), (3, 5, 260)]
KINDS = ["weickert", "exponential", "rational"]
DIAG, OFF = (0, 3, 5), (1, 2, 4)


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def image(shape):
    return 100.0 * synth.image(shape, seed=9)


_REF = {}


def ref(shape):
    """The restatement's gradient (fp64 and emulated fp32) and s, once per shape and left
    unchanged."""
    if shape not in _REF:
        g = np.stack(P.gradient(image(shape), SP, SIGMA))
        g32 = np.stack(P.gradient_fp32(image(shape), SP, SIGMA))
        r = dict(g=g, g32=g32, s=P.magnitude(g), s32=P.magnitude_fp32(g32))
        for a in r.values():
            a.setflags(write=False)
        r["K"] = P.row_contrast(r["s"])
        _REF[shape] = r
    return _REF[shape]


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_fp64(M, shape):
    """Measured on an MI355X: 5.5e-16, 7.0e-16, 7.6e-16 of max|g| for the three shapes."""
    v = M.PM(shape, SP, precision=M.FP64, noise_scale=SIGMA)
    G = v.gradient(image(shape))
    v.close()
    assert G.shape == (3,) + shape
    err = relmax(G, ref(shape)["g"])
    print(f"gradient 3D fp64 {shape}: {err:.3e} of max|g|")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_fp32(M, shape):
    """fp32 storage and FIR arithmetic.  Measured on an MI355X: 2.4e-7, 3.6e-7, 4.2e-7 of max|g|
    against bounds 1.1e-6, 1.4e-6, 1.5e-6 (4 x the emulation's 2.9e-7, 3.6e-7, 3.6e-7)."""
    r = ref(shape)
    bound = 4.0 * relmax(r["g32"], r["g"])
    v = M.PM(shape, SP, precision=M.FP32, noise_scale=SIGMA)
    G = v.gradient(image(shape))
    v.close()
    err = relmax(G, r["g"])
    print(f"gradient 3D fp32 {shape}: {err:.3e} of max|g|, bound {bound:.3e}")
    assert 0.0 < bound < 1e-5
    assert err <= bound


def spread_floor(shape, kind):
    """What the restated g must reach below.  0.2 everywhere but one row: the 60 voxels of
    (3, 4, 5) have s in [8.24, 261.3], and the rational function cannot span that: g > 0.9 at
    s = 8.24 needs K^2 > 73, g < 0.2 at s = 261.3 needs K^2 < 62.  That row asserts 0.3 (the
    median contrast gives 0.268)."""
    return 0.3 if (shape, kind) == ((3, 4, 5), "rational") else 0.2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_tensor_matches_restatement(M, precision, kind):
    """The contrast of each shape is its median gradient magnitude (pm_numpy.row_contrast: 9.61,
    4.94, 6.41), which spreads the restated g over [<= 0.2, >= 0.9] (spread_floor names the one
    row where no contrast can).  Measured max|g - ref| on an MI355X, shapes in SHAPES order (the
    three diagonals and the diffusivity output are the same bits):
      fp64 weickert 1.0e-15, 3.6e-15, 2.0e-15;  exponential 4.4e-16, 1.9e-15, 1.2e-15;
           rational 3.9e-16, 1.3e-15, 8.9e-16
      fp32 weickert 3.3e-7, 1.4e-6, 1.0e-6 against bounds 1.5e-6, 5.8e-6, 4.3e-6;
           exponential 1.9e-7, 7.9e-7, 6.1e-7 against 8.0e-7, 4.4e-6, 2.3e-6;
           rational 1.4e-7, 5.7e-7, 4.2e-7 against 5.5e-7, 3.1e-6, 1.7e-6"""
    for shape in SHAPES:
        r = ref(shape)
        kw = dict(contrast=r["K"], exponent=2.0, alpha=0.01)
        gr = P.diffusivity(r["s"], P.NAMES[kind], **kw)
        assert gr.min() < spread_floor(shape, kind) and gr.max() > 0.9, (shape, gr.min(), gr.max())
        if precision == "FP64":
            bound = 1e-12
        else:
            bound = 4.0 * np.abs(P.diffusivity(r["s32"], P.NAMES[kind], **kw) - gr).max()
            assert 0.0 < bound <= 1e-3
        v = M.PM(shape, SP, precision=getattr(M, precision), diffusivity=kind, noise_scale=SIGMA, **kw)
        D, g = v.tensor(image(shape), with_diffusivity=True)
        D_only = v.tensor(image(shape))
        v.close()
        assert D.shape == (6,) + shape and g.shape == shape
        err = np.abs(g - gr).max()
        print(f"tensor 3D {precision} {kind} {shape}: K = {r['K']:.3f}, g in [{gr.min():.4f}, {gr.max():.4f}], "
              f"max|g - ref| = {err:.3e}, bound {bound:.3e}")
        # structure: exact zeros off the diagonal, one set of bits on it and in the diffusivity
        for c in OFF:
            assert not D[c].any() and not np.signbit(D[c]).any(), c
        for c in DIAG:
            assert D[c].tobytes() == g.tobytes(), c
        assert D_only.tobytes() == D.tobytes()
        assert np.abs(D - P.tensor_from_diffusivity(gr)).max() == err
        assert err <= bound


@pytest.mark.parametrize("exponent", [1.0, 1.5, 3.0])
def test_other_exponents(M, exponent):
    """m = 1, the pow branch (1.5, 3): Weickert, fp64 on (3, 5, 260), <= 1e-12 absolute (measured
    1.3e-15, 1.8e-15, 3.0e-15)."""
    shape = (3, 5, 260)
    r = ref(shape)
    kw = dict(contrast=r["K"], exponent=exponent, alpha=0.01)
    v = M.PM(shape, SP, precision=M.FP64, noise_scale=SIGMA, **kw)
    D, g = v.tensor(image(shape), with_diffusivity=True)
    v.close()
    gr = P.diffusivity(r["s"], P.WEICKERT, **kw)
    err = np.abs(g - gr).max()
    print(f"tensor 3D fp64 weickert m = {exponent}: max|g - ref| = {err:.3e}, g in [{gr.min():.4f}, {gr.max():.4f}]")
    assert D[0].tobytes() == g.tobytes()
    assert err <= 1e-12


@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_constant_image_gives_identity(M, precision):
    """s is a few roundings of the storage precision squared, far below K^2 = 25."""
    shape = (5, 6, 70)
    for kind in KINDS if precision == "FP64" else ["weickert"]:
        v = M.PM(shape, SP, precision=getattr(M, precision), diffusivity=kind, noise_scale=SIGMA, contrast=5.0)
        D = v.tensor(np.full(shape, 42.0))
        v.close()
        for c in range(6):
            err = np.abs(D[c] - (1.0 if c in DIAG else 0.0)).max()
            print(f"constant 3D {precision} {kind} component {c}: {err:.3e}")
            assert err <= 1e-12, (kind, c)


def test_too_long_taps(M):
    """fp64 storage: sigma = 9.6 gives radius ceil(4 x 9.6 / 1.25) = 31 along z, one past what the
    z pass's smallest tile holds ((4 + 2 x 31) x 256 x 8 B = 132 KiB > 128 KiB).
    MAD_ERR_UNSUPPORTED with a message, again on a second call; sigma = 9.3 (radius 30) runs."""
    shape = (3, 4, 5)
    img = image(shape)
    assert P.radii(9.6, SP)[2] == 31 and (4 + 2 * 31) * 256 * 8 > P.LDS_CAP
    assert P.radii(9.3, SP)[2] == 30 and (4 + 2 * 30) * 256 * 8 <= P.LDS_CAP
    v = M.PM(shape, SP, precision=M.FP64, noise_scale=9.6)
    for call in (v.gradient, v.tensor, v.run):
        with pytest.raises(M.MadError) as e:
            call(img)
        print(f"taps too long: {e.value}")
        assert e.value.code == M.capi.ERR_UNSUPPORTED
        assert "taps too long" in str(e.value)
    v.close()
    v = M.PM(shape, SP, precision=M.FP64, noise_scale=9.3)
    G = v.gradient(img)
    v.close()
    err = relmax(G, np.stack(P.gradient(img, SP, 9.3)))
    print(f"radius 30 along z: {err:.3e} of max|g|")
    assert err <= 1e-12


FILTER_SHAPE = (10, 12, 14)
FILTER_KW = dict(noise_scale=SIGMA, contrast=5.0, exponent=2.0, alpha=0.01, diffusion_iterations=2,
                 time_step=0.5, tolerance=1e-10)


def oracle_steps(oracle_mod, x, T, kw):
    o = oracle_mod.Oracle(x.shape, SP, T, kw["time_step"])
    return o.run(x, cycle=oracle_mod.VCYCLE, smoother=oracle_mod.GS_LEX, iterations_per_grid=2,
                 max_cycles=100, number_of_steps=kw["diffusion_iterations"], tolerance=kw["tolerance"])[0]


@pytest.mark.parametrize("shape,kind", [(FILTER_SHAPE, "weickert"), (FILTER_SHAPE, "exponential"),
                                        ((24, 26, 28), "weickert")])
def test_filter_fp64_matches_restatement_and_oracle(M, oracle_mod, shape, kind):
    """Two outer iterations of two implicit steps, iteration by iteration, against the
    restatement's tensor fed to the C oracle: <= 1e-8 of max|ref|.  (10, 12, 14) is a single
    level, one direct solve per step (measured: weickert 3.1e-15 and 5.0e-15, exponential
    2.5e-15 and 4.8e-15, 2 and 4 cycles); (24, 26, 28), the CED filter test's shape, runs the
    multigrid cycle on the isotropic operator (measured 5.0e-11 and
    9.5e-11, 10 and 20 cycles)."""
    img = image(shape)
    refs, _ = P.pm_run(img, SP, oracle_mod, iterations=2, diffusivity=P.NAMES[kind], **FILTER_KW)
    for its in (1, 2):
        v = M.PM(shape, SP, precision=M.FP64, iterations=its, diffusivity=kind, **FILTER_KW)
        out, st = v.run(img)
        v.close()
        err = relmax(out, refs[its - 1])
        print(f"filter 3D fp64 {shape} {kind} iteration {its}: {err:.3e} of max|ref|, cycles {st['total_cycles']}")
        assert st["iterations"] == its and st["total_cycles"] >= 2 * its
        assert err <= 1e-8


def test_filter_fp32_matches_oracle_on_its_own_tensor(M, oracle_mod):
    """fp32: each outer iteration's solve against the oracle run on the GPU's own tensor of
    that iteration's input: <= 1e-5 of max|ref| (measured 8.0e-8 and 5.5e-8)."""
    img = image(FILTER_SHAPE)
    v1 = M.PM(FILTER_SHAPE, SP, precision=M.FP32, iterations=1, **FILTER_KW)
    v2 = M.PM(FILTER_SHAPE, SP, precision=M.FP32, iterations=2, **FILTER_KW)
    out1, _ = v1.run(img)
    out2, st2 = v2.run(img)
    ref1 = oracle_steps(oracle_mod, img, v1.tensor(img), FILTER_KW)
    ref2 = oracle_steps(oracle_mod, out1, v1.tensor(out1), FILTER_KW)
    v1.close()
    v2.close()
    e1, e2 = relmax(out1, ref1), relmax(out2, ref2)
    print(f"filter 3D fp32: iteration 1 {e1:.3e}, iteration 2 {e2:.3e} of max|ref|")
    assert st2["iterations"] == 2
    assert e1 <= 1e-5 and e2 <= 1e-5


@pytest.mark.parametrize("precision", ["PRECISION_AUTO", "FP64"])
def test_two_iterations_equal_two_chained_runs(M, precision):
    img = image(FILTER_SHAPE)
    kw = dict(FILTER_KW, tolerance=1e-6, precision=getattr(M, precision))
    v = M.PM(FILTER_SHAPE, SP, iterations=2, **kw)
    both, st = v.run(img)
    v.close()
    v = M.PM(FILTER_SHAPE, SP, iterations=1, **kw)
    a, sa = v.run(img)
    b, sb = v.run(a)
    v.close()
    assert st["total_cycles"] == sa["total_cycles"] + sb["total_cycles"]
    np.testing.assert_array_equal(both, b)


def test_keeps_the_edge_and_smooths_the_flats(M):
    """A noisy step of 50 along x in a volume: Perona-Malik (time step 2, 2 x 2 steps) keeps more
    of the jump than the identity tensor over the same 4 steps (measured 20.59 of 49.89 against
    5.59; the restatement + oracle give 20.59), and the flat regions come out smoother than they
    went in (standard deviation 1.95 -> 0.31).  Rational diffusivity, sigma = 1.5:
    pm_numpy.monotonicity is 0.53 <= 1, so the output stays within the input's range (see the
    2D test of this name)."""
    shape = (8, 10, 24)
    rng = np.random.default_rng(3)
    x = np.arange(shape[2])
    img = np.where(x >= 12, 150.0, 100.0) + rng.normal(0.0, 2.0, size=shape)
    sp = (1.0, 1.0, 1.0)
    mono = P.monotonicity(P.pm_tensor(img, sp, P.RATIONAL, 1.5, 5.0, 2.0, 0.01)[1])
    print(f"monotonicity of the first tensor: {mono:.3f}")
    assert mono <= 1.0
    v = M.PM(shape, sp, diffusivity="rational", noise_scale=1.5, contrast=5.0, alpha=0.01, time_step=2.0,
             iterations=2, diffusion_iterations=2)
    out, _ = v.run(img)
    v.close()
    s = M.Solver(shape, sp, time_step=2.0, number_of_steps=4)
    I = np.zeros((6,) + shape)
    I[0] = I[3] = I[5] = 1.0
    s.set_tensor(I)
    iso, _ = s.run(img, out_dtype=np.float64)
    s.close()
    jump = lambda u: float((u[..., 12] - u[..., 11]).mean())
    print(f"jump: input {jump(img):.2f}, Perona-Malik {jump(out):.2f}, identity {jump(iso):.2f}")
    assert jump(out) > jump(iso)
    flat = lambda u: max(u[..., :8].std(), u[..., 16:].std())
    print(f"flat std: input {flat(img):.3f}, Perona-Malik {flat(out):.3f}")
    assert flat(out) < flat(img)
    print(f"range: input [{img.min():.2f}, {img.max():.2f}], Perona-Malik [{out.min():.2f}, {out.max():.2f}]")
    assert img.min() <= out.min() and out.max() <= img.max()


def test_facade(M):
    vol = image((8, 9, 10)).astype(np.float32)
    f = M.PeronaMalikDiffusionImageFilter.New()
    f.SetInput(M.Image(vol, spacing=SP, origin=(1.0, 2.0, 3.0)))
    f.SetDiffusivity("exponential")
    f.SetNoiseScale(0.7)
    f.SetConductanceParameter(5.0)
    f.SetAlpha(0.02)
    f.SetNumberOfIterations(2)
    f.SetDiffusionIterations(2)
    f.SetTimeStep(0.2)
    out = f.Update()
    assert out is f.GetOutput()
    assert out.GetBufferAsArray().dtype == np.float32 and out.GetBufferAsArray().shape == vol.shape
    assert out.spacing == SP and out.origin == (1.0, 2.0, 3.0)
    assert (out.GetBufferAsArray() != vol).any()
    st = f.stats
    assert st["iterations"] == 2 and st["total_cycles"] >= 4 and st["converged"]
    assert len(st["pass_ms"]) == 3 and all(t > 0.0 for t in st["pass_ms"])
    assert abs(st["tensor_ms"] - sum(st["pass_ms"])) <= 1e-9 * st["tensor_ms"]
    assert st["tile"] == (0, 0) and st["diffusion_ms"] > 0.0
