"""Per-kernel parity with the fp64 oracle on ragged multi-tile shapes, at every level.

The golden fixtures stop at 28 points per axis and the ved2 crop at 55: one x tile, so no
oracle comparison there crosses an x tile seam, takes a ragged last x tile, runs the
diagonal-tensor instances of the tiled kernels, or looks at a coarse operator on its own.
The shapes below do (ROWS, checked on the CPU by test_rows_cross_what_they_claim), and every
kernel-level entry point is compared with the oracle at every level l < num_levels - 1: the
oracle is computed here, once per row, and shared by the tests.

Tolerances (the project's, tests/test_gpu_kernels.py)
  fp64: max|gpu - ref| <= 1e-12 max|ref| for single kernels, 1e-14 for transfers, the
        residual norm within 1e-12 relative, one V-cycle 1e-10.
  fp32: transfers 4 eps32 of max|ref|; GS sweeps 64 eps32 of max|ref|; one V-cycle 2e-5;
        WJ and the residual pointwise |gpu - ref| <= 16 eps32 mag, with
        mag = |b| + D|x| + sum |coef| |x_nb| from the matrix-free coefficients at level 0 of
        the 3D rows (the tight form of test_gpu_kernels.stencil_mag) and
        mag_i = |b_i| + (sum_j |S_ij|) max|x| from the oracle's own stencil S elsewhere.
        Inputs are uniform on [0.5, 1.5), which keeps the second form within 3x of the first.
  No fp32 case needed a measured bound: every one holds the bounds above.
"""
import collections
import zlib

import numpy as np
import pytest

import mf_numpy as mf
import synth

EPS32 = np.finfo(np.float32).eps
SPACING = (1.0, 0.8, 1.3)  # x first, as the bitwise tests of test_gpu_kernels.py
DT = 0.7

# Tile constants of the launch sites in csrc/mad_solver.hip, restated:
TX, TY = 64, 16   # launch_wj, residual_impl: wj3_k / resid3_k columns (3D levels of >= 16 x 16)
CX, CY = 32, 8    # restrict_arr: restrict3_k coarse columns
IX, IY = 64, 16   # launch_interp3: interp3_k fine columns, IX * VX points wide;
#                   VX = 2 where nx (and with it the row and plane strides) is even, else 1
BX, BY = 64, 4    # BLK: the per-point kernels' block (2D levels, 3D levels under 16 x 16)
MIN_TILED = 16    # launch_wj, residual_impl: nx, ny >= 16 take the tiled kernels


def split(n, tile):
    """Widths of the tiles that cover n points."""
    return tuple(min(tile, n - i) for i in range(0, n, tile))


def z_chunks(nz, tiles, target=1024, zdiv=8):
    """launch_wj / residual_impl: z chunks sized for ~1024 blocks, at least 8 planes each."""
    chunks = max(1, min((target + tiles - 1) // tiles, nz // zdiv))
    return split(nz, (nz + chunks - 1) // chunks)


# per level l: the tile widths the row is there for.  x / y: smoother and residual tiles
# (TX x TY, or BX x BY on the per-point path); ix: interpolation tiles of the fine level l
# (IX * vx); rx: restriction tiles of the coarse level l (CX); z: smoother z chunks
Row = collections.namedtuple("Row", "shape tensor ncolors coarse cross")
ROWS = {
    "full134": Row((24, 37, 134), "full", 4, [(12, 19, 67), (6, 10, 34)], {
        0: dict(tiled=True, x=(64, 64, 6), y=(16, 16, 5), vx=2, ix=(128, 6)),
        1: dict(tiled=True, x=(64, 3), vx=1, ix=(64, 3), rx=(32, 32, 3))}),
    "odd131": Row((33, 35, 131), "full", 4, [(17, 18, 66), (9, 9, 33)], {
        0: dict(tiled=True, x=(64, 64, 3), y=(16, 16, 3), z=(9, 9, 9, 6), vx=1, ix=(64, 64, 3)),
        1: dict(tiled=True, x=(64, 2), vx=2, rx=(32, 32, 2), centering=[0, 0, 0])}),
    "wide262": Row((48, 35, 262), "full", 4, [(24, 18, 131), (12, 9, 66)], {
        0: dict(tiled=True, x=(64, 64, 64, 64, 6), vx=2, ix=(128, 128, 6)),
        1: dict(tiled=True, x=(64, 64, 3), vx=1, ix=(64, 64, 3), rx=(32, 32, 32, 32, 3))}),
    "diag66": Row((70, 40, 66), "diag", 2, [(35, 20, 33), (18, 10, 17)], {
        0: dict(tiled=True, x=(64, 2), y=(16, 16, 8), z=(9, 9, 9, 9, 9, 9, 9, 7), vx=2),
        1: dict(tiled=True, vx=1, rx=(32, 1))}),
    "iso129": Row((33, 65, 129), "iso", 2, [(17, 33, 65), (9, 17, 33)], {
        0: dict(tiled=True, x=(64, 64, 1), y=(16, 16, 16, 16, 1), z=(9, 9, 9, 6), vx=1,
                ix=(64, 64, 1)),
        1: dict(tiled=True, x=(64, 1), y=(16, 16, 1), vx=1, ix=(64, 1), rx=(32, 32, 1))}),
    "full2d": Row((37, 150), "full", 4, None, {
        0: dict(tiled=False, x=(64, 64, 22), y=(4,) * 9 + (1,)),
        1: dict(tiled=False, x=(64, 11), y=(4, 4, 4, 4, 3))}),
}
ROWS3D = [n for n in ROWS if len(ROWS[n].shape) == 3]


class Ctx:
    """One row's oracle, inputs and references: built once, shared, never written to."""

    def __init__(self, oracle_mod, name):
        row = ROWS[name]
        self.name, self.row, self.om = name, row, oracle_mod
        shape = row.shape
        self.dim = len(shape)
        self.spacing = SPACING[: self.dim]
        self.T = {"full": lambda: synth.random_spd(shape, seed=1),
                  "diag": lambda: synth.random_spd(shape, seed=1, offdiag=False),
                  "iso": lambda: synth.isotropic(shape)}[row.tensor]()
        self.o = oracle_mod.Oracle(shape, self.spacing, self.T, DT)
        self._cache = {}

    def rng(self, tag, l):
        return np.random.default_rng(zlib.crc32(f"{self.name}/{tag}/{l}".encode()))

    def get(self, kind, l):
        key = (kind, l)
        if key not in self._cache:
            v = getattr(self, "_" + kind)(l)
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            self._cache[key] = v
        return self._cache[key]

    # inputs: uniform on [0.5, 1.5) for the stencil kernels, standard normal for transfers
    def _x(self, l):
        return self.rng("x", l).uniform(0.5, 1.5, self.o.shape_at(l))

    def _b(self, l):
        return self.rng("b", l).uniform(0.5, 1.5, self.o.shape_at(l))

    def _fine(self, l):
        return self.rng("fine", l).standard_normal(self.o.shape_at(l))

    def _coarse(self, l):  # an array of level l + 1, the input of interpolate(l)
        return self.rng("coarse", l).standard_normal(self.o.shape_at(l + 1))

    # references
    def _residual(self, l):
        return self.o.residual(l, self.get("x", l), self.get("b", l))

    def _wj(self, l):
        return self.o.wj(l, self.get("x", l), self.get("b", l))

    def _gs(self, l):
        return self.o.gs_color(l, self.get("x", l), self.get("b", l), ncolors=self.row.ncolors)

    def _restrict(self, l):
        return self.o.restrict(l, self.get("fine", l))

    def _interp(self, l):
        return self.o.interpolate(l, self.get("coarse", l))

    def _vcycle_gs(self, l):
        return self.o.vcycle(self.get("x", 0), self.get("b", 0), smoother=self.om.GS_COLOR,
                             ncolors=self.row.ncolors)

    def _vcycle_wj(self, l):
        return self.o.vcycle(self.get("x", 0), self.get("b", 0), smoother=self.om.WJ)

    # fp32 rounding magnitudes of the residual (mag) and the operator's diagonal
    def _mag_diag(self, l):
        x, b = self.get("x", l), self.get("b", l)
        if l == 0 and self.dim == 3:
            co = mf.coefficients(self.T, self.spacing, DT)
            aco = dict(a=[np.abs(v) for v in co["a"]], g=[np.abs(v) for v in co["g"]],
                       e={k: np.abs(v) for k, v in co["e"].items()})
            # |a+g| + |a-g| <= 2(|a| + |g|), as test_gpu_kernels.stencil_mag
            return (np.abs(b) + mf.diag(co) * np.abs(x) + 2.0 * mf.off_sum(np.abs(x), aco),
                    mf.diag(co))
        S = self.o.stencil(l)
        shape = self.o.shape_at(l)
        return (np.abs(b) + np.abs(S).sum(axis=1).reshape(shape) * np.abs(x).max(),
                S[:, 13].reshape(shape))


@pytest.fixture(scope="module")
def ctx_of(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ctx(oracle_mod, name)
        return cache[name]
    yield get
    cache.clear()  # the oracles go before the interpreter shuts down


@pytest.fixture(params=["fp32", "fp64"])
def prec(request):
    import multigridanisotropicdiffusion_amd as M
    return M.FP32 if request.param == "fp32" else M.FP64


def relmax(a, ref):
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


# ----------------------------------------------------------------- CPU: the table itself

@pytest.mark.parametrize("name", list(ROWS))
def test_rows_cross_what_they_claim(name, ctx_of, oracle_mod):
    """Each row still has the level shapes the table states, the GPU level plan (host-only
    mad_plan_level / mad_max_depth) gives the oracle's, and at those shapes every claimed axis
    has more than one tile with a ragged last one, the parity of nx selects the claimed
    interpolation form, and the levels claimed tiled have nx, ny >= 16."""
    import multigridanisotropicdiffusion_amd as M
    from multigridanisotropicdiffusion_amd import distributed as D
    c = ctx_of(name)
    row, o = c.row, c.o
    levels = [o.shape_at(l) for l in range(o.num_levels)]
    assert levels[0] == row.shape
    if row.coarse is not None:
        assert levels[1:] == row.coarse
    plan = D.plan(row.shape)
    assert [tuple(reversed(p["size"][: c.dim])) for p in plan] == levels
    assert not any(p["distributed"] for p in plan)
    assert M.max_depth(row.shape) == oracle_mod.max_depth(row.shape) == len(levels) - 1
    assert sorted(row.cross) == list(range(len(levels) - 1))  # every level but the coarsest

    def ragged(widths, tile):
        return len(widths) > 1 and widths[-1] < tile and all(w == tile for w in widths[:-1])

    for l, claim in row.cross.items():
        ny, nx = levels[l][-2:]
        tiled = c.dim == 3 and nx >= MIN_TILED and ny >= MIN_TILED
        assert tiled == claim["tiled"], (l, nx, ny)
        tx, ty = (TX, TY) if tiled else (BX, BY)
        if "x" in claim:
            assert split(nx, tx) == claim["x"] and ragged(claim["x"], tx), l
        if "y" in claim:
            assert split(ny, ty) == claim["y"] and ragged(claim["y"], ty), l
        if "z" in claim:
            nz = levels[l][0]
            zs = z_chunks(nz, len(split(nx, tx)) * len(split(ny, ty)))
            assert zs == claim["z"] and len(zs) > 1 and zs[-1] < zs[0], l
        if "vx" in claim:
            assert claim["vx"] == (2 if nx % 2 == 0 else 1), (l, nx)
        if "ix" in claim:
            assert split(nx, IX * claim["vx"]) == claim["ix"] and ragged(claim["ix"], IX * claim["vx"]), l
        if "rx" in claim:  # level l as the coarse side of restrict(l - 1)
            assert l >= 1 and split(nx, CX) == claim["rx"] and ragged(claim["rx"], CX), l
        if "centering" in claim:
            assert o.levels[l]["centering"] == claim["centering"], l


def test_table_covers_every_form():
    """Across the rows: both interpolation forms with a ragged last x tile, x seams in the
    tiled kernels of every tensor kind, an x seam at a level >= 1, ragged z chunks."""
    claims = [(r.tensor, l, cl) for r in ROWS.values() for l, cl in r.cross.items() if cl["tiled"]]
    assert {cl["vx"] for _, _, cl in claims if "ix" in cl} == {1, 2}
    assert {t for t, _, cl in claims if "x" in cl} == {"full", "diag", "iso"}
    assert any(l >= 1 and "x" in cl for _, l, cl in claims)
    assert any("z" in cl for _, _, cl in claims)
    assert any("rx" in cl for _, _, cl in claims)


# ----------------------------------------------------------------- GPU

def make_solver(c, prec, **kw):
    import multigridanisotropicdiffusion_amd as M
    s = M.Solver(c.row.shape, c.spacing, time_step=DT, precision=prec, **kw)
    s.set_tensor(c.T)
    s.setup()
    assert s.num_levels == c.o.num_levels
    assert [s.shape_at(l) for l in range(s.num_levels)] == [c.o.shape_at(l) for l in range(s.num_levels)]
    return s


def check_wj_and_residual(c, s, prec, l, brec):
    import multigridanisotropicdiffusion_amd as M
    x, b = c.get("x", l), c.get("b", l)
    kname = s.smooth_kernel_name(l)
    if c.row.cross[l]["tiled"]:
        assert kname.startswith("wj3_k<") and kname.endswith(("true>" if brec else "false>")), kname
    else:
        assert kname.startswith("wj_k<"), kname
    s.upload(l, M.capi.X, x)
    s.upload(l, M.capi.B, b)
    nrm = s.residual(l)
    r = s.download(l, M.capi.R)
    s.smooth(l, 1)
    wj = s.download(l, M.capi.X)
    rref, wref = c.get("residual", l), c.get("wj", l)
    if prec == M.FP64:
        er, ew = relmax(r, rref), relmax(wj, wref)
        en = abs(nrm - np.linalg.norm(rref)) / np.linalg.norm(rref)
        print(f"{c.name} l={l} fp64 residual {er:.2e} wj {ew:.2e} norm {en:.2e} (bound 1e-12)")
        assert er < 1e-12, l
        assert ew < 1e-12, l
        assert en < 1e-12, l
    else:
        mag, dg = c.get("mag_diag", l)
        er = (np.abs(r - rref) / mag).max() / EPS32
        ew = (np.abs(wj - wref) / (mag / dg + np.abs(x))).max() / EPS32
        en = abs(nrm - np.linalg.norm(r)) / np.linalg.norm(r)
        print(f"{c.name} l={l} fp32 residual {er:.2f} eps wj {ew:.2f} eps (bound 16), norm {en:.2e}")
        assert er < 16, l
        assert ew < 16, l
        assert en < 1e-6, l


def check_gs(c, s, prec, l, gs_kernel):
    import multigridanisotropicdiffusion_amd as M
    kname = s.smooth_kernel_name(l)
    fused = gs_kernel == 3 and c.dim == 3
    assert kname.startswith("gs_fused3_k<" if fused else "gs_color_k<"), kname
    s.upload(l, M.capi.X, c.get("x", l))
    s.upload(l, M.capi.B, c.get("b", l))
    s.smooth(l, 1)
    e = relmax(s.download(l, M.capi.X), c.get("gs", l))
    print(f"{c.name} l={l} gs_kernel={gs_kernel} {kname}: {e:.2e}")
    assert e < (1e-12 if prec == M.FP64 else 64 * EPS32), l


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROWS))
def test_wj_and_residual_every_level(name, prec, ctx_of):
    """residual(l) (array and norm) and one WJ sweep at every level against the oracle's:
    wj3_k / resid3_k of every tensor kind across x, y tile seams and ragged last tiles, the
    coarse operators on their own, and the per-point kernels in 2D."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)
    s = make_solver(c, prec, smoother=M.WEIGHTED_JACOBI)
    for l in range(s.num_levels - 1):
        check_wj_and_residual(c, s, prec, l, brec=False)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("gs_kernel", [1, 3])
@pytest.mark.parametrize("name", list(ROWS))
def test_gs_sweep_every_level(name, prec, gs_kernel, ctx_of):
    """One multicolour GS sweep at every level, per-colour passes (gs_kernel 1) and the fused
    single launch (3), against the oracle's sweep in the same colour order (4 colours for the
    full tensor, red-black for diagonal / isotropic)."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)
    s = make_solver(c, prec, smoother=M.GAUSS_SEIDEL, gs_kernel=gs_kernel)
    for l in range(s.num_levels - 1):
        check_gs(c, s, prec, l, gs_kernel)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["wj", "gs1", "gs3"])
@pytest.mark.parametrize("name", ["full134", "diag66"])
def test_level0_with_b_in_the_records(name, prec, mode, ctx_of):
    """cycle=SMOOTHER: the level-0 coefficient records carry b (the BREC instances of wj3_k,
    resid3_k and both GS forms); the same level-0 comparisons as above."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)
    if mode == "wj":
        s = make_solver(c, prec, smoother=M.WEIGHTED_JACOBI, cycle=M.capi.SMOOTHER)
        check_wj_and_residual(c, s, prec, 0, brec=True)
    else:
        s = make_solver(c, prec, smoother=M.GAUSS_SEIDEL, gs_kernel=int(mode[2]), cycle=M.capi.SMOOTHER)
        if mode == "gs3":  # "... 2, BREC, PEER, BL, ZU, BS>"
            assert ", 2, true, " in s.smooth_kernel_name(0), s.smooth_kernel_name(0)
        check_gs(c, s, prec, 0, int(mode[2]))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ROWS))
def test_transfers_every_level(name, prec, ctx_of):
    """restrict(l), interpolate(l) and prolongate_add(l) of random arrays at every level with
    several tiles per axis: restrict3_k over 32-wide coarse tiles, interp3_k in its scalar
    (odd nx) and two-points-per-thread (even nx) forms, writing and adding."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)
    s = make_solver(c, prec, smoother=M.GAUSS_SEIDEL)
    tol = 1e-14 if prec == M.FP64 else 4 * EPS32
    for l in range(s.num_levels - 1):
        if "vx" in c.row.cross[l]:  # the form launch_interp3 takes at this level
            assert (2 if s.shape_at(l)[-1] % 2 == 0 else 1) == c.row.cross[l]["vx"], l
        s.upload(l, M.capi.R, c.get("fine", l))
        s.restrict(l)
        er = relmax(s.download(l + 1, M.capi.B), c.get("restrict", l))
        s.upload(l + 1, M.capi.X, c.get("coarse", l))
        s.interpolate(l)
        ei = relmax(s.download(l, M.capi.X), c.get("interp", l))
        s.upload(l, M.capi.X, c.get("x", l))
        s.prolongate_add(l)
        ea = relmax(s.download(l, M.capi.X), c.get("x", l) + c.get("interp", l))
        print(f"{c.name} l={l} restrict {er:.2e} interpolate {ei:.2e} prolongate_add {ea:.2e} (bound {tol:.1e})")
        assert er < tol, l
        assert ei < tol, l
        assert ea < tol, l
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("smoother_key", ["gs", "wj"])
@pytest.mark.parametrize("name", list(ROWS))
def test_one_vcycle(name, prec, smoother_key, ctx_of):
    """One V-cycle (nu = 2) with the oracle's smoother and colour order: the pieces above
    together at these shapes."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)
    s = make_solver(c, prec, smoother=M.GAUSS_SEIDEL if smoother_key == "gs" else M.WEIGHTED_JACOBI)
    s.upload(0, M.capi.X, c.get("x", 0))
    s.upload(0, M.capi.B, c.get("b", 0))
    s.vcycle()
    e = relmax(s.download(0, M.capi.X), c.get("vcycle_" + smoother_key, 0))
    s.close()
    print(f"{c.name} vcycle {smoother_key}: {e:.2e}")
    assert e < (1e-10 if prec == M.FP64 else 2e-5)
