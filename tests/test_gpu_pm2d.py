"""2D regularised Perona-Malik diffusion on the GPU (include/mad_pm.h, dim = 2: the fused
kernel pm2_k) against the fp64 numpy restatement (tests/pm_numpy.py) and the C MAD oracle.

Every comparison prints its figure before asserting (pytest -s shows them).  The bounds:
  gradient: fp64 <= 1e-12 of max|g| (the kernel sums its taps in the restatement's order);
    fp32 <= 4 x the error of pm_numpy.gradient_fp32, a plain-numpy fp32 emulation of step 1 that
    shares nothing with the kernel, against the fp64 restatement (the margin is for fma against
    multiply-add and for tap-order effects).
  tensor / diffusivity: fp64 <= 1e-12 absolute; fp32 <= 4 x the error of the emulated fp32
    gradient pushed through the fp64 map, and under the project's ceiling 1e-3.
  whole filter: fp64 <= 1e-8 of max|ref| against the restatement + oracle; fp32 <= 1e-5 against
    the oracle run on the GPU's own tensor (the CED bars).
"""
import numpy as np
import pytest

import pm_numpy as P
import synth

pytestmark = pytest.mark.gpu

SP = (0.8, 1.25)
SIGMA = 1.0  # radii 5 / 4 along x / y
# (6, 7): every halo is longer than its axis (all indices clamped); (9, 65): off the 64-lane
# width; (70, 300): crosses tile seams in both axes with the halo over each seam.  The tile is
# at most 64 columns x 32 rows, so no further shape is needed to cross it.
SHAPES = [(6, 7), (9, 65), (70, 300)]
KINDS = ["weickert", "exponential", "rational"]


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def image(shape):
    return 100.0 * synth.image(shape, seed=9)


_REF = {}


def ref(shape, sigma=SIGMA):
    """The restatement's gradient (fp64 and emulated fp32) and s, once per (shape, sigma) and left
    unchanged."""
    key = (shape, sigma)
    if key not in _REF:
        g = np.stack(P.gradient(image(shape), SP, sigma))
        g32 = np.stack(P.gradient_fp32(image(shape), SP, sigma))
        r = dict(g=g, g32=g32, s=P.magnitude(g), s32=P.magnitude_fp32(g32))
        for a in r.values():
            a.setflags(write=False)
        r["K"] = P.row_contrast(r["s"])
        _REF[key] = r
    return _REF[key]


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_fp64(M, shape):
    """Measured on an MI355X: 5.2e-16, 5.8e-16, 6.2e-16 of max|g| for the three shapes."""
    v = M.PM2D(shape, SP, precision=M.FP64, noise_scale=SIGMA)
    G = v.gradient(image(shape))
    v.close()
    assert G.shape == (2,) + shape
    err = relmax(G, ref(shape)["g"])
    print(f"gradient 2D fp64 {shape}: {err:.3e} of max|g|")
    assert err <= 1e-12


@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_fp32(M, shape):
    """fp32 storage and FIR arithmetic.  Measured on an MI355X: 2.4e-7, 3.9e-7, 2.7e-7 of max|g|
    against bounds 8.7e-7, 1.3e-6, 1.2e-6 (4 x the emulation's 2.2e-7, 3.2e-7, 2.9e-7)."""
    r = ref(shape)
    bound = 4.0 * relmax(r["g32"], r["g"])
    v = M.PM2D(shape, SP, precision=M.FP32, noise_scale=SIGMA)
    G = v.gradient(image(shape))
    v.close()
    err = relmax(G, r["g"])
    print(f"gradient 2D fp32 {shape}: {err:.3e} of max|g|, bound {bound:.3e}")
    assert 0.0 < bound < 1e-5
    assert err <= bound


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_tensor_matches_restatement(M, precision, kind):
    """The contrast of each shape is its median gradient magnitude (pm_numpy.row_contrast: 12.06,
    6.82, 6.88), which spreads the restated g over [<= 0.2, >= 0.9] for every diffusivity.
    Measured max|g - ref| on an MI355X, shapes in SHAPES order (D[0] and the diffusivity output
    are the same bits):
      fp64 weickert 1.2e-15, 1.2e-15, 1.9e-15;  exponential 7.2e-16, 8.9e-16, 1.6e-15;
           rational 4.4e-16, 7.8e-16, 1.2e-15
      fp32 weickert 4.5e-7, 5.8e-7, 1.1e-6 against bounds 1.8e-6, 2.8e-6, 4.3e-6;
           exponential 2.4e-7, 5.2e-7, 6.1e-7 against 9.6e-7, 2.1e-6, 3.2e-6;
           rational 1.7e-7, 4.2e-7, 4.7e-7 against 6.6e-7, 1.5e-6, 2.3e-6"""
    for shape in SHAPES:
        r = ref(shape)
        kw = dict(contrast=r["K"], exponent=2.0, alpha=0.01)
        gr = P.diffusivity(r["s"], P.NAMES[kind], **kw)
        assert gr.min() < 0.2 and gr.max() > 0.9, (shape, gr.min(), gr.max())
        if precision == "FP64":
            bound = 1e-12
        else:
            bound = 4.0 * np.abs(P.diffusivity(r["s32"], P.NAMES[kind], **kw) - gr).max()
            assert 0.0 < bound <= 1e-3
        v = M.PM2D(shape, SP, precision=getattr(M, precision), diffusivity=kind, noise_scale=SIGMA, **kw)
        D, g = v.tensor(image(shape), with_diffusivity=True)
        D_only = v.tensor(image(shape))
        v.close()
        assert D.shape == (3,) + shape and g.shape == shape
        err = np.abs(g - gr).max()
        print(f"tensor 2D {precision} {kind} {shape}: K = {r['K']:.3f}, g in [{gr.min():.4f}, {gr.max():.4f}], "
              f"max|g - ref| = {err:.3e}, bound {bound:.3e}")
        # structure: exact zeros off the diagonal, one set of bits on it and in the diffusivity
        assert not D[1].any() and not np.signbit(D[1]).any()
        assert D[0].tobytes() == D[2].tobytes() == g.tobytes()
        assert D_only.tobytes() == D.tobytes()
        assert np.abs(D - P.tensor_from_diffusivity(gr)).max() == err
        assert err <= bound


@pytest.mark.parametrize("exponent", [1.0, 1.5, 3.0])
def test_other_exponents(M, exponent):
    """The kernel takes (K^2 / s)^m without pow for m = 2 (every other test here) and m = 1; these
    run the other branches, Weickert, fp64 on (9, 65): <= 1e-12 absolute (measured 8.9e-16,
    1.2e-15, 1.3e-15)."""
    shape = (9, 65)
    r = ref(shape)
    kw = dict(contrast=r["K"], exponent=exponent, alpha=0.01)
    v = M.PM2D(shape, SP, precision=M.FP64, noise_scale=SIGMA, **kw)
    D, g = v.tensor(image(shape), with_diffusivity=True)
    v.close()
    gr = P.diffusivity(r["s"], P.WEICKERT, **kw)
    err = np.abs(g - gr).max()
    print(f"tensor 2D fp64 weickert m = {exponent}: max|g - ref| = {err:.3e}, g in [{gr.min():.4f}, {gr.max():.4f}]")
    assert D[0].tobytes() == g.tobytes()
    assert err <= 1e-12


@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_constant_image_gives_identity(M, precision):
    """s is a few roundings of the storage precision squared, far below K^2 = 25."""
    shape = (10, 70)
    for kind in KINDS if precision == "FP64" else ["weickert"]:
        v = M.PM2D(shape, SP, precision=getattr(M, precision), diffusivity=kind, noise_scale=SIGMA,
                   contrast=5.0)
        D = v.tensor(np.full(shape, 42.0))
        v.close()
        for c, want in enumerate((1.0, 0.0, 1.0)):
            err = np.abs(D[c] - want).max()
            print(f"constant 2D {precision} {kind} component {c}: {err:.3e}")
            assert err <= 1e-12, (kind, c)


def test_weickert_diffusivity_equals_eeds_eigenvalue_on_a_ramp(M):
    """u = a x + b y (physical coordinates), fp64.  At least R_sigma + R_rho from every border no
    tap of either scale is clamped: the structure tensor is the constant rank-one
    (a, b)(a, b)^T, mu1 - mu0 = a^2 + b^2 = |grad u_sigma|^2, and the existing 2D EED kernel's
    across-edge eigenvalue lam[1] is the Weickert diffusivity.  Both also equal the analytic
    1 - (1 - alpha) h(a^2 + b^2).  <= 1e-12 (measured: EED against PM 7.8e-16, PM against the
    analytic value 8.9e-16, EED 6.7e-16)."""
    shape, a, b, rho = (30, 36), 3.0, -2.0, 1.0
    kw = dict(noise_scale=SIGMA, contrast=3.5, exponent=2.0, alpha=0.01)
    y, x = np.mgrid[:shape[0], :shape[1]]
    img = a * x * SP[0] + b * y * SP[1]
    v = M.PM2D(shape, SP, precision=M.FP64, **kw)
    _, g = v.tensor(img, with_diffusivity=True)
    v.close()
    c = M.CED2D(shape, SP, precision=M.FP64, enhancement="eed", feature_scale=rho, **kw)
    _, lam = c.tensor(img, with_lambda=True)
    c.close()
    (Rx, Ry), (Qx, Qy) = P.radii(SIGMA, SP), P.radii(rho, SP)
    inner = (slice(Ry + Qy, shape[0] - Ry - Qy), slice(Rx + Qx, shape[1] - Rx - Qx))
    assert g[inner].size >= 100
    s = a * a + b * b
    want = 1.0 - (1.0 - kw["alpha"]) * np.exp(-(kw["contrast"] ** 2 / s) ** kw["exponent"])
    e_cross = np.abs(lam[1][inner] - g[inner]).max()
    e_pm, e_eed = np.abs(g[inner] - want).max(), np.abs(lam[1][inner] - want).max()
    print(f"ramp: analytic g = {want:.6f}; EED lam1 - PM g {e_cross:.3e}, PM - analytic {e_pm:.3e}, "
          f"EED - analytic {e_eed:.3e}")
    assert 0.2 < want < 0.9
    assert e_cross <= 1e-12 and e_pm <= 1e-12 and e_eed <= 1e-12


def test_transposed_image_transposes_the_result(M):
    """Image (y, x) -> (x, y) with the spacing swapped: the phases run along the other axis with
    the other radii; gx <-> gy, g transposes.  fp64, <= 1e-9 (measured: gradient 1.1e-14
    absolute, g 2.2e-15)."""
    shape = (26, 30)
    img = image(shape)
    kw = dict(precision=M.FP64, noise_scale=SIGMA, contrast=7.0)
    v = M.PM2D(shape, SP, **kw)
    G = v.gradient(img)
    _, g = v.tensor(img, with_diffusivity=True)
    v.close()
    v = M.PM2D(shape[::-1], SP[::-1], **kw)
    Gt = v.gradient(np.ascontiguousarray(img.T))
    _, gt = v.tensor(np.ascontiguousarray(img.T), with_diffusivity=True)
    v.close()
    eg = max(np.abs(Gt[1] - G[0].T).max(), np.abs(Gt[0] - G[1].T).max())
    ed = np.abs(gt - g.T).max()
    print(f"transpose 2D: gradient {eg:.3e}, g {ed:.3e}")
    assert eg <= 1e-9 and ed <= 1e-9


def test_reduced_tile_and_too_long_taps(M):
    """fp64 storage, the sigmas of pm_numpy.TILE_TABLE_FP64 (proved from the LDS arithmetic in
    tests/test_pm_cpu.py::test_tile_plan): sigma = 1 takes the full 64 x 32 tile, sigma = 4 (radii
    20 / 13) 64 x 16; (40, 90) crosses the reduced tile's seams in both axes.  Parity of the
    gradient <= 1e-12 of max|g| (measured 5.0e-16 and 1.2e-15).  sigma = 14.25 (radii 72 / 46) needs 135680 B at
    the floor tile 16 x 4: MAD_ERR_UNSUPPORTED with a message, again on a second call, and a
    supported context used before and after returns the same bits."""
    shape = (40, 90)
    img = image(shape)
    for sigma in (1.0, 4.0):
        v = M.PM2D(shape, SP, precision=M.FP64, noise_scale=sigma, contrast=5.0, diffusion_iterations=1)
        G = v.gradient(img)
        _, st = v.run(img)
        if sigma == 4.0:
            before = v.tensor(img)
            ok = v
        else:
            v.close()
        err = relmax(G, ref(shape, sigma)["g"])
        print(f"reduced tile: sigma {sigma} tile {st['tile']}: {err:.3e} of max|g|")
        assert st["tile"] == P.TILE_TABLE_FP64[sigma]
        assert err <= 1e-12
    assert P.TILE_TABLE_FP64[14.25] is None
    bad = M.PM2D(shape, SP, precision=M.FP64, noise_scale=14.25)
    for call in (bad.gradient, bad.tensor, bad.run):
        with pytest.raises(M.MadError) as e:
            call(img)
        print(f"taps too long: {e.value}")
        assert e.value.code == M.capi.ERR_UNSUPPORTED
        assert "taps too long" in str(e.value)
    bad.close()
    after = ok.tensor(img)
    ok.close()
    assert after.tobytes() == before.tobytes()


FILTER_SHAPE = (26, 28)
FILTER_KW = dict(noise_scale=SIGMA, contrast=7.0, exponent=2.0, alpha=0.01, diffusion_iterations=2,
                 time_step=0.5, tolerance=1e-10)


def oracle_steps(oracle_mod, x, T, kw, spacing=SP):
    o = oracle_mod.Oracle(x.shape, spacing, T, kw["time_step"])
    return o.run(x, cycle=oracle_mod.VCYCLE, smoother=oracle_mod.GS_LEX, iterations_per_grid=2,
                 max_cycles=100, number_of_steps=kw["diffusion_iterations"], tolerance=kw["tolerance"])[0]


@pytest.mark.parametrize("kind", ["weickert", "rational"])
def test_filter_fp64_matches_restatement_and_oracle(M, oracle_mod, kind):
    """Two outer iterations of two implicit steps, iteration by iteration, against the
    restatement's tensor fed to the C oracle: <= 1e-8 of max|ref| (measured: weickert 1.5e-11
    and 8.7e-11, 8 and 16 cycles; rational 2.0e-10 and 1.4e-10, 8 and 16 cycles)."""
    img = image(FILTER_SHAPE)
    refs, _ = P.pm_run(img, SP, oracle_mod, iterations=2, diffusivity=P.NAMES[kind], **FILTER_KW)
    for its in (1, 2):
        v = M.PM2D(FILTER_SHAPE, SP, precision=M.FP64, iterations=its, diffusivity=kind, **FILTER_KW)
        out, st = v.run(img)
        v.close()
        err = relmax(out, refs[its - 1])
        print(f"filter 2D fp64 {kind} iteration {its}: {err:.3e} of max|ref|, cycles {st['total_cycles']}")
        assert st["iterations"] == its and st["total_cycles"] >= 2 * its
        assert err <= 1e-8


def test_filter_fp32_matches_oracle_on_its_own_tensor(M, oracle_mod):
    """fp32: each outer iteration's solve against the oracle run on the GPU's own tensor of
    that iteration's input: <= 1e-5 of max|ref| (measured 2.0e-7 and 1.7e-7)."""
    img = image(FILTER_SHAPE)
    v1 = M.PM2D(FILTER_SHAPE, SP, precision=M.FP32, iterations=1, **FILTER_KW)
    v2 = M.PM2D(FILTER_SHAPE, SP, precision=M.FP32, iterations=2, **FILTER_KW)
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


@pytest.mark.parametrize("precision", ["PRECISION_AUTO", "FP64"])
def test_two_iterations_equal_two_chained_runs(M, precision):
    img = image(FILTER_SHAPE)
    kw = dict(FILTER_KW, tolerance=1e-6, precision=getattr(M, precision))
    v = M.PM2D(FILTER_SHAPE, SP, iterations=2, **kw)
    both, st = v.run(img)
    v.close()
    v = M.PM2D(FILTER_SHAPE, SP, iterations=1, **kw)
    a, sa = v.run(img)
    b, sb = v.run(a)
    v.close()
    assert st["total_cycles"] == sa["total_cycles"] + sb["total_cycles"]
    np.testing.assert_array_equal(both, b)


BEHAVIOUR_KW = dict(diffusivity="rational", noise_scale=1.5, contrast=5.0, alpha=0.01)


def test_keeps_the_edge_and_smooths_the_flats(M):
    """A noisy step of 50 along x: Perona-Malik (time step 2, 2 x 2 steps) keeps more of the jump
    than the identity tensor over the same 4 steps (measured 20.51 of 49.66 against 5.58; the
    restatement + oracle give 20.51), and the flat regions come out smoother than they went in
    (standard deviation 1.97 -> 0.39).  The rational diffusivity at sigma = 1.5 keeps
    pm_numpy.monotonicity at 0.53 <= 1, inside the range where the solver's stencil is an
    M-matrix, so the output also stays within the input's range (DESIGN.md "Nonlinear isotropic
    diffusion (Perona-Malik)", monotonicity: the default Weickert diffusivity at sigma = 0.7 and
    K = 5 reaches 21 on this image and overshoots, on the GPU as in the oracle)."""
    shape = (20, 24)
    rng = np.random.default_rng(3)
    x = np.arange(shape[1])
    img = np.where(x >= 12, 150.0, 100.0) + rng.normal(0.0, 2.0, size=shape)
    sp = (1.0, 1.0)
    mono = P.monotonicity(P.pm_tensor(img, sp, P.RATIONAL, 1.5, 5.0, 2.0, 0.01)[1])
    print(f"monotonicity of the first tensor: {mono:.3f}")
    assert mono <= 1.0
    v = M.PM2D(shape, sp, time_step=2.0, iterations=2, diffusion_iterations=2, **BEHAVIOUR_KW)
    out, _ = v.run(img)
    v.close()
    s = M.Solver(shape, sp, time_step=2.0, number_of_steps=4)
    I = np.zeros((3,) + shape)
    I[0] = I[2] = 1.0
    s.set_tensor(I)
    iso, _ = s.run(img, out_dtype=np.float64)
    s.close()
    jump = lambda u: float((u[:, 12] - u[:, 11]).mean())
    print(f"jump: input {jump(img):.2f}, Perona-Malik {jump(out):.2f}, identity {jump(iso):.2f}")
    assert jump(out) > jump(iso)
    flat = lambda u: max(u[:, :8].std(), u[:, 16:].std())
    print(f"flat std: input {flat(img):.3f}, Perona-Malik {flat(out):.3f}")
    assert flat(out) < flat(img)
    print(f"range: input [{img.min():.2f}, {img.max():.2f}], Perona-Malik [{out.min():.2f}, {out.max():.2f}]")
    assert img.min() <= out.min() and out.max() <= img.max()


def test_facade(M):
    shape = (14, 16)
    img = np.round(image(shape)).astype(np.int16)
    f = M.PeronaMalikDiffusionImageFilter()
    f.SetInput(M.Image(img, spacing=SP, origin=(1.0, 2.0)))
    f.SetDiffusivity("rational")
    f.SetNoiseScale(0.7)
    f.SetConductanceParameter(6.0)
    f.SetExponent(2.0)
    f.SetAlpha(0.02)
    f.SetNumberOfIterations(2)
    f.SetDiffusionIterations(2)
    f.SetTimeStep(0.2)
    f.SetTolerance(1e-6)
    f.SetCycle(f.VCYCLE)
    f.SetDiffusionIterationsPerGrid(2)
    f.SetVerbose(False)
    assert f._p["contrast"] == 6.0 and f._p["iterations"] == 2 and f._p["diffusivity"] == M.capi.PM_RATIONAL
    f.SetContrast(5.0)
    f.SetIterations(2)
    out = f.Update()
    assert out is f.GetOutput()
    assert out.GetBufferAsArray().dtype == np.int16 and out.GetBufferAsArray().shape == shape
    assert out.spacing == SP and out.origin == (1.0, 2.0)
    assert (out.GetBufferAsArray() != img).any()
    st = f.stats
    assert st["iterations"] == 2 and st["total_cycles"] >= 4 and st["converged"]
    assert len(st["pass_ms"]) == 3 and st["pass_ms"][0] > 0.0
    assert st["pass_ms"][1:] == [0.0, 0.0] and st["tensor_ms"] == st["pass_ms"][0]
    assert st["tile"] == (64, 32) and st["diffusion_ms"] > 0.0 and st["stalled"] == 0
    assert set(st) == {"iterations", "total_cycles", "last_relres", "tensor_ms", "diffusion_ms", "pass_ms",
                       "stalled", "tile", "converged"}
