"""Vector-valued Perona-Malik diffusion on the GPU (include/mad_pm.h, "Vector-valued images": the
kernels pm2v_k and pmv_x_k, one joint diffusivity for all channels) against the fp64 numpy
restatement (tests/pm_vector_numpy.py), the C MAD oracle, and the scalar path.

Every comparison prints its figure before asserting (pytest -s shows them).  The bounds are those
of tests/test_gpu_pm2d.py:
  gradient: fp64 <= 1e-12 of max|g|; fp32 <= 4 x the error of the plain-numpy fp32 emulation.
  tensor / diffusivity: fp64 <= 1e-12 absolute; fp32 <= 4 x the error of the emulated fp32 joint s
    pushed through the fp64 map, and under the project's ceiling 1e-3.
  whole filter: fp64 <= 1e-8 of max|ref| against the restatement + oracle; fp32 <= 1e-5 against
    the oracle run on the GPU's own joint tensor.
The anchors to the scalar path are bitwise.

Channel c of a shape is 100 synth.image(shape, seed=9 + c).  Two rows take another first seed:
the 42 pixels of (6, 7) and the 60 voxels of (3, 4, 5) with seed 9 have a joint s that spans a
factor of 8 and 16, and no contrast spreads the rational diffusivity (which needs a factor of 37)
over [<= 0.2, >= 0.9].  Seeds 182 and 27, found on the CPU, are the first at which the restated g
of all three diffusivities spans that range with the median contrast.
"""
import math

import numpy as np
import pytest

import pm_numpy as P
import pm_vector_numpy as V
import synth

pytestmark = pytest.mark.gpu

SIGMA = 1.0
SP = {2: (0.8, 1.25), 3: (0.8, 1.0, 1.25)}
CH = {2: 3, 3: 2}
# the parity shapes of tests/test_gpu_pm2d.py and tests/test_gpu_pm.py
SHAPES = {2: [(6, 7), (9, 65), (70, 300)], 3: [(3, 4, 5), (34, 35, 70), (3, 5, 260)]}
FIRST_SEED = {(6, 7): 182, (3, 4, 5): 27}
KINDS = ["weickert", "exponential", "rational"]
PARITY = [(d, s) for d in (2, 3) for s in SHAPES[d]]
# the shapes of the anchors and of quantile mode: both cross every tile seam
SEAM = {2: (70, 300), 3: (34, 35, 70)}
FILTER_SHAPE = {2: (26, 28), 3: (10, 12, 14)}
FILTER_KW = {2: dict(noise_scale=SIGMA, contrast=7.0, exponent=2.0, alpha=0.01, diffusion_iterations=2,
                     time_step=0.5, tolerance=1e-10),
             3: dict(noise_scale=SIGMA, contrast=5.0, exponent=2.0, alpha=0.01, diffusion_iterations=2,
                     time_step=0.5, tolerance=1e-10)}


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def ctx(M, shape, **kw):
    kw.setdefault("noise_scale", SIGMA)
    return (M.PM2D if len(shape) == 2 else M.PM)(shape, SP[len(shape)], **kw)


def image(shape, channels=None):
    channels = channels or CH[len(shape)]
    return np.stack([100.0 * synth.image(shape, seed=FIRST_SEED.get(shape, 9) + c) for c in range(channels)])


_REF = {}


def ref(shape, sigma=SIGMA, channels=None):
    """The restatement's per-channel gradients (fp64 and emulated fp32) and joint s, once per case
    and left unchanged."""
    key = (shape, sigma, channels)
    if key not in _REF:
        img, sp = image(shape, channels), SP[len(shape)]
        g, g32 = V.gradients(img, sp, sigma), V.gradients_fp32(img, sp, sigma)
        r = dict(g=g, g32=g32, s=V.joint_s(g), s32=V.joint_s_fp32(g32))
        for a in r.values():
            a.setflags(write=False)
        r["K"] = P.row_contrast(r["s"])
        _REF[key] = r
    return _REF[key]


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def own_s(v, img, precision):
    """The joint s of the GPU's own gradient by step 2's rule (the gradient output holds the
    storage values exactly)."""
    G = v.gradient(img)
    return V.joint_s(G) if precision == "FP64" else V.joint_s_fp32(G)


def structure(D, g):
    """Exact zeros off the diagonal, one set of bits on it and in the diffusivity."""
    diag = (0, 2) if D.shape[0] == 3 else (0, 3, 5)
    for c in range(D.shape[0]):
        if c in diag:
            assert D[c].tobytes() == g.tobytes(), c
        else:
            assert not D[c].any() and not np.signbit(D[c]).any(), c


# ------------------------------------------------------------------ parity with the restatement

@pytest.mark.parametrize("dim,shape", PARITY)
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_gradient(M, precision, dim, shape):
    """Measured on an MI355X, of max|g|: fp64 4.3e-16 .. 7.6e-16; fp32 1.8e-7, 3.5e-7, 3.2e-7 (2D) and
    2.4e-7, 3.6e-7, 4.2e-7 (3D) against bounds 9.1e-7, 1.3e-6, 1.2e-6 and 1.0e-6, 1.5e-6, 1.7e-6."""
    r = ref(shape)
    v = ctx(M, shape, precision=getattr(M, precision), channels=CH[dim])
    G = v.gradient(image(shape))
    v.close()
    assert G.shape == (CH[dim], dim) + shape
    err = relmax(G, r["g"])
    if precision == "FP64":
        bound = 1e-12
    else:
        bound = 4.0 * relmax(r["g32"], r["g"])
        assert 0.0 < bound < 1e-5
    print(f"gradient {dim}D {precision} {shape} C = {CH[dim]}: {err:.3e} of max|g|, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_tensor_matches_restatement(M, precision, kind, dim):
    """The contrast of each shape is the median of the joint |grad u| (2D 15.28, 13.96, 13.43; 3D
    14.13, 7.40, 9.65).  Measured max|g - ref| on an MI355X over the three shapes of a dimension:
      fp64  2D weickert <= 1.1e-15, exponential <= 5.6e-16, rational <= 4.4e-16;
            3D weickert <= 2.1e-15, exponential <= 1.1e-15, rational <= 7.8e-16
      fp32  2D weickert 2.8e-7, 3.1e-7, 7.2e-7 against bounds 9.6e-7, 1.4e-6, 2.5e-6;
            3D weickert 4.0e-7, 8.0e-7, 6.2e-7 against 1.5e-6, 4.2e-6, 2.8e-6; the other two
            diffusivities lie below Weickert's figures and keep the same factor of 3-5 to their bounds"""
    for shape in SHAPES[dim]:
        r = ref(shape)
        kw = dict(contrast=r["K"], exponent=2.0, alpha=0.01)
        gr = P.diffusivity(r["s"], P.NAMES[kind], **kw)
        assert gr.min() <= 0.2 and gr.max() >= 0.9, (shape, gr.min(), gr.max())
        if precision == "FP64":
            bound = 1e-12
        else:
            bound = 4.0 * np.abs(P.diffusivity(r["s32"], P.NAMES[kind], **kw) - gr).max()
            assert 0.0 < bound <= 1e-3
        v = ctx(M, shape, precision=getattr(M, precision), diffusivity=kind, channels=CH[dim], **kw)
        D, g = v.tensor(image(shape), with_diffusivity=True)
        D_only = v.tensor(image(shape))
        v.close()
        assert D.shape == (dim * (dim + 1) // 2,) + shape and g.shape == shape
        err = np.abs(g - gr).max()
        print(f"tensor {dim}D {precision} {kind} {shape}: K = {r['K']:.3f}, g in [{gr.min():.4f}, {gr.max():.4f}], "
              f"max|g - ref| = {err:.3e}, bound {bound:.3e}")
        structure(D, g)
        assert D_only.tobytes() == D.tobytes()
        assert err <= bound


# ------------------------------------------------------------------ bitwise anchors to the scalar path

@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_tensor_anchors_to_the_scalar_path(M, precision, dim):
    """a. (u, 0): exact zeros give s_1 = 0 and s_0 + 0 = s_0 -- the scalar tensor's bits.
    b. (u, u) with K^2 doubled: s + s = 2 s, and the power of two cancels in every diffusivity.
    d. (u, w) and (w, u): the sum of two terms commutes."""
    shape = SEAM[dim]
    u, w = image(shape, 2)
    k2 = ref(shape, channels=2)["K"] ** 2 / 2.0
    for kind in KINDS:
        kw = dict(precision=getattr(M, precision), diffusivity=kind, alpha=0.01)
        s = ctx(M, shape, _contrast_squared=k2, **kw)
        Ds = s.tensor(u)
        s.close()
        v = ctx(M, shape, channels=2, _contrast_squared=k2, **kw)
        Da = v.tensor(np.stack([u, np.zeros_like(u)]))
        Duw, Dwu = v.tensor(np.stack([u, w])), v.tensor(np.stack([w, u]))
        v.close()
        v = ctx(M, shape, channels=2, _contrast_squared=2.0 * k2, **kw)
        Db = v.tensor(np.stack([u, u]))
        v.close()
        print(f"anchors {dim}D {precision} {kind}: g in [{Ds[0].min():.4f}, {Ds[0].max():.4f}], "
              f"(u, w) differs from u in {int((Duw[0] != Ds[0]).sum())} of {u.size}")
        assert Ds[0].min() < 0.5 < Ds[0].max()
        assert Da.tobytes() == Ds.tobytes()
        assert Db.tobytes() == Ds.tobytes()
        assert Duw.tobytes() == Dwu.tobytes()
        assert (Duw[0] != Ds[0]).any()


@pytest.mark.parametrize("shape", [FILTER_SHAPE[2], FILTER_SHAPE[3], (24, 26, 28)])
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_run_on_equal_channels_is_the_scalar_run(M, precision, shape):
    """c. On (u, u) with K^2 doubled both channels of run come out equal to each other and to the
    scalar run on u, bit for bit: the second channel's steps on the first channel's setup equal
    steps on a fresh one.  Two outer iterations.  (10, 12, 14) is a single level, one direct solve
    per step; (26, 28) and (24, 26, 28) run the multigrid cycle on the reused operators.
    Measured on an MI355X: 2D 18 cycles against the scalar run's 9, (10, 12, 14) 8 against 4."""
    dim = len(shape)
    u = image(shape, 1)[0]
    kw = dict(FILTER_KW[dim], precision=getattr(M, precision), iterations=2, tolerance=1e-6)
    k2 = kw.pop("contrast") ** 2
    s = ctx(M, shape, _contrast_squared=k2, **kw)
    want, ss = s.run(u)
    s.close()
    v = ctx(M, shape, channels=2, _contrast_squared=2.0 * k2, **kw)
    out, st = v.run(np.stack([u, u]))
    v.close()
    print(f"equal channels {shape} {precision}: cycles {st['total_cycles']} (scalar {ss['total_cycles']}), "
          f"relres {st['last_relres']:.3e} (scalar {ss['last_relres']:.3e})")
    assert out.shape == (2,) + shape and st["channels"] == 2 and "channels" not in ss
    assert out[0].tobytes() == out[1].tobytes() == want.tobytes()
    assert st["total_cycles"] == 2 * ss["total_cycles"] and st["last_relres"] == ss["last_relres"]
    assert (want != u).any()


# ------------------------------------------------------------------ quantile mode

@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("precision", ["FP64", "FP32"])
def test_quantile_mode_selects_on_the_joint_s(M, precision, dim):
    shape, q = SEAM[dim], 0.9
    img = image(shape)
    for kind in KINDS:
        kw = dict(precision=getattr(M, precision), diffusivity=kind, alpha=0.01, channels=CH[dim])
        v = ctx(M, shape, contrast_quantile=q, diffusion_iterations=1, **kw)
        s_gpu = own_s(v, img, precision)
        K = v.contrast(img, q)
        D, g = v.tensor(img, with_diffusivity=True)
        _, st = v.run(img)
        v.close()
        k2 = float(np.quantile(s_gpu, q, method="inverted_cdf"))
        k2_ref = float(np.quantile(ref(shape)["s"], q, method="inverted_cdf"))
        err = abs(k2 - k2_ref) / k2_ref
        print(f"quantile {dim}D {precision} {kind}: K = {K:.6f}, |s_q - s_q(ref)| / s_q(ref) = {err:.3e}")
        assert K == math.sqrt(k2) == st["contrast_used"]
        if precision == "FP64":
            assert err <= 1e-12
            assert relmax(s_gpu, ref(shape)["s"]) <= 1e-12
        a = ctx(M, shape, _contrast_squared=k2, **kw)
        Da, ga = a.tensor(img, with_diffusivity=True)
        a.close()
        assert g.min() < 0.5 < g.max()
        assert D.tobytes() == Da.tobytes() and g.tobytes() == ga.tobytes()
        structure(D, g)


# ------------------------------------------------------------------ the whole filter

@pytest.mark.parametrize("dim", [2, 3])
def test_filter_fp64_matches_restatement_and_oracle(M, oracle_mod, dim):
    """Two outer iterations of two implicit steps per channel, iteration by iteration, against the
    restatement's joint tensor fed to the C oracle: <= 1e-8 of max|ref| (measured on an MI355X: 2D
    4.0e-10 and 3.3e-10 with 18 and 36 cycles; 3D, a single level, 3.7e-15 and 4.6e-15)."""
    shape, kw = FILTER_SHAPE[dim], FILTER_KW[dim]
    img = image(shape)
    refs = V.pm_run(img, SP[dim], oracle_mod, iterations=2, diffusivity=P.WEICKERT, **kw)
    for its in (1, 2):
        v = ctx(M, shape, precision=M.FP64, iterations=its, channels=CH[dim], **kw)
        out, st = v.run(img)
        v.close()
        err = relmax(out, refs[its - 1])
        print(f"filter {dim}D fp64 iteration {its}: {err:.3e} of max|ref|, cycles {st['total_cycles']}")
        assert st["iterations"] == its and st["total_cycles"] >= 2 * its * CH[dim]
        assert err <= 1e-8


@pytest.mark.parametrize("dim", [2, 3])
def test_filter_fp32_matches_oracle_on_its_own_tensor(M, oracle_mod, dim):
    """fp32: each outer iteration's solves against the oracle run, channel by channel, on the GPU's
    own joint tensor of that iteration's input: <= 1e-5 of max|ref| (measured on an MI355X: 2D
    2.0e-7 and 1.5e-7, 3D 9.9e-8 and 6.7e-8)."""
    shape, kw = FILTER_SHAPE[dim], FILTER_KW[dim]
    img = image(shape)
    p = dict(P.DEFAULTS, **kw)
    v1 = ctx(M, shape, precision=M.FP32, iterations=1, channels=CH[dim], **kw)
    v2 = ctx(M, shape, precision=M.FP32, iterations=2, channels=CH[dim], **kw)
    out1, _ = v1.run(img)
    out2, st2 = v2.run(img)
    ref1, _ = V.oracle_steps(oracle_mod, img, v1.tensor(img), SP[dim], p)
    ref2, _ = V.oracle_steps(oracle_mod, out1, v1.tensor(out1), SP[dim], p)
    v1.close()
    v2.close()
    e1, e2 = relmax(out1, ref1), relmax(out2, ref2)
    print(f"filter {dim}D fp32: iteration 1 {e1:.3e}, iteration 2 {e2:.3e} of max|ref|")
    assert st2["iterations"] == 2
    assert e1 <= 1e-5 and e2 <= 1e-5


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("precision", ["PRECISION_AUTO", "FP64"])
def test_two_iterations_equal_two_chained_runs(M, precision, dim):
    shape = FILTER_SHAPE[dim]
    img = image(shape)
    kw = dict(FILTER_KW[dim], tolerance=1e-6, precision=getattr(M, precision), channels=CH[dim])
    v = ctx(M, shape, iterations=2, **kw)
    both, st = v.run(img)
    v.close()
    v = ctx(M, shape, iterations=1, **kw)
    a, sa = v.run(img)
    b, sb = v.run(a)
    v.close()
    print(f"chained {dim}D {precision}: cycles {st['total_cycles']} = {sa['total_cycles']} + {sb['total_cycles']}")
    assert st["total_cycles"] == sa["total_cycles"] + sb["total_cycles"]
    np.testing.assert_array_equal(both, b)


def test_a_strong_edge_protects_a_weak_one(M, oracle_mod):
    """The case of tests/test_pm_vector_cpu.py on the GPU (default precision), the same assertions;
    in fp64 the jumps are within 1e-6 relative of the restatement + oracle's.  That comparison runs
    both sides at tolerance 1e-10: at the default 1e-6 each solver stops within 1e-6 of the step's
    solution by its own smoother, and the two need not agree to the bar itself."""
    img, sp = V.behaviour_image(), (1.0, 1.0)
    kw = dict(V.BEHAVIOUR_KW, diffusivity="rational")
    v = M.PM2D(V.BEHAVIOUR_SHAPE, sp, channels=2, **kw)
    joint, _ = v.run(img)
    _, g = v.tensor(img, with_diffusivity=True)
    v.close()
    s = M.PM2D(V.BEHAVIOUR_SHAPE, sp, **kw)
    split = np.stack([s.run(img[c])[0] for c in range(2)])
    s.close()
    V.behaviour_checks(img, joint, split, P.monotonicity(g))
    v = M.PM2D(V.BEHAVIOUR_SHAPE, sp, channels=2, precision=M.FP64, tolerance=1e-10, **kw)
    joint64, _ = v.run(img)
    v.close()
    want = V.pm_run(img, sp, oracle_mod, **dict(V.BEHAVIOUR_KW, tolerance=1e-10))[-1]
    for c in range(2):
        a, b = V.jump(joint64[c]), V.jump(want[c])
        print(f"channel {c} jump fp64: GPU {a:.8f}, oracle {b:.8f}, relative {abs(a - b) / abs(b):.3e}")
        assert abs(a - b) <= 1e-6 * abs(b)


# ------------------------------------------------------------------ tiles, limits, layouts

def test_reduced_tile_and_too_long_taps(M):
    """fp64 sigma = 4 (radii 20 / 13) takes the 64 x 16 tile of pm_numpy.TILE_TABLE_FP64 with two
    channels as with one; (40, 90) crosses its seams in both axes.  sigma = 14.25 does not fit the
    floor tile: MAD_ERR_UNSUPPORTED with a message, and a supported context used before and after
    returns the same bits."""
    shape = (40, 90)
    img = image(shape, 2)
    ok = M.PM2D(shape, SP[2], precision=M.FP64, noise_scale=4.0, contrast=5.0, diffusion_iterations=1, channels=2)
    G = ok.gradient(img)
    _, st = ok.run(img)
    before = ok.tensor(img)
    err = relmax(G, ref(shape, 4.0, 2)["g"])
    print(f"reduced tile: sigma 4 tile {st['tile']}: {err:.3e} of max|g|")
    assert st["tile"] == (64, 16) == P.TILE_TABLE_FP64[4.0]
    assert err <= 1e-12
    bad = M.PM2D(shape, SP[2], precision=M.FP64, noise_scale=14.25, channels=2)
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


def test_channel_axis_round_trips_the_layout(M):
    shape = (14, 16)
    img = image(shape, 3)
    kw = dict(noise_scale=0.7, contrast=6.0, diffusion_iterations=2, time_step=0.2, channels=3)
    v = M.PM2D(shape, SP[2], **kw)
    first, _ = v.run(img)
    last, st = v.run(np.moveaxis(img, 0, -1), channel_axis=-1)
    v.close()
    assert first.shape == (3,) + shape and last.shape == shape + (3,) and last.flags["C_CONTIGUOUS"]
    assert st["channels"] == 3
    assert np.array_equal(np.moveaxis(last, -1, 0), first)
    assert (first != img).any()


def test_facade_runs_a_colour_picture(M):
    shape = (14, 16)
    planar = np.round(image(shape, 3)).astype(np.int16)
    pic = np.ascontiguousarray(np.moveaxis(planar, 0, -1))
    f = M.PeronaMalikDiffusionImageFilter()
    f.SetInput(M.Image(pic, spacing=SP[2], origin=(1.0, 2.0)), channel_axis=-1)
    f.SetDiffusivity("rational")
    f.SetNoiseScale(0.7)
    f.SetContrast(6.0)
    f.SetIterations(2)
    f.SetDiffusionIterations(2)
    f.SetTimeStep(0.2)
    out = f.Update()
    a = out.GetBufferAsArray()
    assert a.dtype == np.int16 and a.shape == shape + (3,)
    assert out.spacing == SP[2] and out.origin == (1.0, 2.0)
    assert (a != pic).any()
    assert f.stats["channels"] == 3 and f.stats["iterations"] == 2 and f.stats["total_cycles"] >= 12
    # the same through the context, channel first
    v = M.PM2D(shape, SP[2], diffusivity="rational", noise_scale=0.7, contrast=6.0, iterations=2,
               diffusion_iterations=2, time_step=0.2, channels=3)
    want, _ = v.run(planar, out_dtype=np.int16)
    v.close()
    assert np.array_equal(np.moveaxis(a, -1, 0), want)
