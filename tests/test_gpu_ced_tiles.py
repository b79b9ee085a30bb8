"""3D structure-tensor (EED / CED) tensor generation across tile seams, over radii and on
designed structure tensors.

tests/test_gpu_ced.py runs one set of radii (Rs = (4, 3, 3), Rr = (10, 8, 7)), compares the
tensor path on single-tile shapes only and never takes ced_generate's tile-halving loops or its
MAD_ERR_UNSUPPORTED path.  The rows below (ROWS, checked on the CPU by
test_rows_cross_what_they_claim and test_table_covers_every_form) cross the 64 x 4 column blocks
of ced_z_k, the 64-column blocks of ced_y_k / ced_ry_k / ced_rz_k, the 256-wide rows of ced_x_k,
the halved z / y tiles that long taps force (ZT, YT, YR, ZR down to its floor of 4), an LDS
request just under the cap, a radius of 1 and halos longer than their axes.  On every row the
structure tensor, the tensor and the mapped eigenvalues (both enhancements, the precisions the
row supports) are compared with tests/ced_numpy.py, the fp64 restatement that shares nothing
with the kernels (LAPACK eigh, VO.correlate); the mapped eigenvalues are also compared with the
eigenvalues of the returned tensor itself.  The eigen-analysis of ced_point is steered with
linear ramps whose structure tensor a a^T is known (RAMP_CASES); the MAD_ERR_UNSUPPORTED path
and what it leaves behind follow.

The library reports its tiles only in 2D (mad_ced_stats.tile), so ced_generate's tile choice is
restated here (ced_plan, KVED_LDS, the block shapes and copy counts): a change of those constants
in csrc/mad_ced.hpp is NOT noticed by this module -- the rows would silently stop crossing what
they claim.  Whoever changes them updates ced_plan with them.

One reference J per row is computed once, write-protected and shared (the refs fixture), with its
eigen-decomposition; the tensor references are CN.eigenvalue_map on that shared decomposition,
which test_shared_reference_is_ced_numpy pins to CN.tensor_from_structure bit for bit.

Each row has its own image and contrast (Row.amp, Row.contrast), chosen on the CPU from the
reference alone so that the mapped eigenvalue that varies (EED lam_2, CED lam_0) reaches down to
0.2 and up to 0.9 on the row: with one contrast for all rows the long-scale rows have a nearly
constant J and a lambda of exactly 1 or alpha, which would hide a wrong eigenvalue map.

Every comparison prints its figure before asserting (pytest -s shows them).  The bounds:
  structure tensor: fp64 <= 1e-12 of max|J| (the project's bar, tests/test_gpu_ced.py);
    fp32 <= TOL_J32 of max|J| = 4 x the largest error measured on an MI355X over the rows, under
    test_gpu_ced.py's ceiling of 10 x the CPU fp32 emulation figure 4.2e-7.
  tensor and lambda: fp64 <= 1e-12 absolute (the bar that pins an fp64 eigen-analysis to eigh in
    tests/test_gpu_ced2d.py); fp32 <= TOL_D32 absolute = 4 x the largest measured, ceiling 1e-3.
  lambda against eigh of the returned D: 1e-12 in both precisions -- the eigen-analysis and
    D = sum lam_i v_i v_i^T are fp64 in every mode, V is orthonormal to rounding, and an
    eigenvalue moves by at most the 2-norm of the perturbation (Weyl).
"""
import collections

import numpy as np
import pytest

import ced_numpy as CN

PRECS = ("fp32", "fp64")
SIZE = {"fp32": 4, "fp64": 8}
ENH = {"eed": CN.EED, "ced": CN.CED}
ALPHA = 0.01

# csrc/mad_ced.hpp, restated (see the module docstring):
KVED_LDS = 131072      # kVedLds: the dynamic LDS cap of the passes
PREFER_LDS = 65536     # ced_rz_k: tiles of <= 64 KiB are preferred (two blocks on a CU)
ZCOLS, ZROWS = 64, 4   # ced_z_k: a block's columns and rows (64 columns also in y, ry, rz)
XROW = 256             # ced_x_k: points of a row per block
COPIES = dict(z=1, y=2, ry=1, rz=6, x_in=3, x_prod=6)  # volumes held in LDS per pass


def split(n, tile):
    """Widths of the tiles that cover n points."""
    return tuple(min(tile, n - i) for i in range(0, n, tile))


def ragged(widths, tile):
    return len(widths) > 1 and widths[-1] < tile and all(w == tile for w in widths[:-1])


Plan = collections.namedtuple("Plan", "Rs Rr ZT YT YR ZR lds fits")


def ced_plan(sigma, rho, spacing, size):
    """ved_taps' radii and ced_generate's tile choice for spacing (x, y, z) and a storage type of
    `size` bytes: Rs, Rr (x, y, z), the tiles ZT (ced_z_k), YT (ced_y_k), YR (ced_ry_k), ZR
    (ced_rz_k), the LDS requests of the five passes in launch order (z, y, x, ry, rz) and
    whether all of them fit the cap."""
    Rs = tuple(max(1, int(np.ceil(4.0 * sigma / h))) for h in spacing)
    Rr = tuple(max(1, int(np.ceil(4.0 * rho / h))) for h in spacing)

    def lds(lines, width, copies):
        return lines * width * copies * size

    ZT = YT = YR = ZR = 32
    while ZT > 4 and lds(ZT + 2 * Rs[2], ZCOLS * ZROWS, COPIES["z"]) > KVED_LDS:
        ZT //= 2
    while YT > 4 and lds(YT + 2 * Rs[1], ZCOLS, COPIES["y"]) > KVED_LDS:
        YT //= 2
    while YR > 4 and lds(YR + 2 * Rr[1], ZCOLS, COPIES["ry"]) > KVED_LDS:
        YR //= 2
    while ZR > 8 and lds(ZR + 2 * Rr[2], ZCOLS, COPIES["rz"]) > PREFER_LDS:
        ZR //= 2
    while ZR > 4 and lds(ZR + 2 * Rr[2], ZCOLS, COPIES["rz"]) > KVED_LDS:
        ZR //= 2
    need = (lds(ZT + 2 * Rs[2], ZCOLS * ZROWS, COPIES["z"]),
            lds(YT + 2 * Rs[1], ZCOLS, COPIES["y"]),
            lds(XROW + 2 * (Rs[0] + Rr[0]), 1, COPIES["x_in"]) + lds(XROW + 2 * Rr[0], 1, COPIES["x_prod"]),
            lds(YR + 2 * Rr[1], ZCOLS, COPIES["ry"]),
            lds(ZR + 2 * Rr[2], ZCOLS, COPIES["rz"]))
    return Plan(Rs, Rr, ZT, YT, YR, ZR, need, all(n <= KVED_LDS for n in need))


# shape (z, y, x), spacing (x, y, z).  claim: the radii Rs, Rr (x, y, z) and, per precision, the
# tiles (ZT, YT, YR, ZR) with the tile widths of every axis the row is there to split (z: ced_z_k,
# y: ced_y_k, yr: ced_ry_k, zr: ced_rz_k; named only where the axis has several tiles with a ragged
# last one) and, where it matters, one pass' LDS request in bytes (lds: pass -> bytes); x:
# ced_x_k's rows; cols: the 64-column blocks; rows4: ced_z_k's 4-row blocks.
# amp, seed: the row's image (row_image); contrast: chosen from the reference J (module docstring).
Row = collections.namedtuple("Row", "shape spacing sigma rho precs seed amp contrast claim")
SP = (0.8, 1.0, 1.25)
ROWS = {
    "seams": Row((37, 70, 300), SP, 0.7, 2.0, PRECS, 31, 1.0, 6.0, dict(
        Rs=(4, 3, 3), Rr=(10, 8, 7),
        fp32=dict(tiles=(32, 32, 32, 16), z=(32, 5), y=(32, 32, 6), yr=(32, 32, 6), zr=(16, 16, 5)),
        fp64=dict(tiles=(32, 32, 32, 8), z=(32, 5), y=(32, 32, 6), yr=(32, 32, 6), zr=(8, 8, 8, 8, 5)),
        x=(256, 44), cols=(64,) * 4 + (44,), rows4=(4,) * 17 + (2,))),
    "longz": Row((21, 9, 70), (1.0, 1.0, 0.5), 2.2, 2.3, PRECS, 32, 1.0, 1.2, dict(
        Rs=(9, 9, 18), Rr=(10, 10, 19),
        fp32=dict(tiles=(32, 32, 32, 8), zr=(8, 8, 5)),
        fp64=dict(tiles=(16, 32, 32, 4), z=(16, 5), zr=(4,) * 5 + (1,), lds=dict(rz=129024)),
        cols=(64, 6), rows4=(4, 4, 1))),
    "longy": Row((9, 37, 70), (1.0, 0.1, 1.0), 1.25, 2.85, PRECS, 33, 1.0, 2.8, dict(
        Rs=(5, 50, 5), Rr=(12, 114, 12),
        fp32=dict(tiles=(32, 32, 32, 16), y=(32, 5), yr=(32, 5)),
        fp64=dict(tiles=(32, 16, 16, 8), y=(16, 16, 5), yr=(16, 16, 5), zr=(8, 1), lds=dict(ry=124928)),
        cols=(64, 6), rows4=(4,) * 9 + (1,))),
    "longy32": Row((9, 37, 70), (1.0, 0.1, 1.0), 2.85, 6.05, ("fp32",), 34, 1.0, 0.6, dict(
        Rs=(12, 114, 12), Rr=(25, 242, 25),
        fp32=dict(tiles=(32, 16, 16, 8), y=(16, 16, 5), yr=(16, 16, 5), zr=(8, 1), lds=dict(ry=128000)),
        cols=(64, 6), rows4=(4,) * 9 + (1,))),
    "longz32": Row((37, 9, 70), (1.0, 1.0, 0.1), 1.25, 1.0, ("fp32",), 35, 1.0, 2.5, dict(
        Rs=(5, 5, 50), Rr=(4, 4, 40),
        fp32=dict(tiles=(16, 32, 32, 4), z=(16, 16, 5), zr=(4,) * 9 + (1,), lds=dict(rz=129024)),
        cols=(64, 6), rows4=(4, 4, 1))),
    "thick": Row((7, 33, 65), (0.5, 0.5, 3.0), 0.7, 2.0, PRECS, 36, 1.0, 7.0, dict(
        Rs=(6, 6, 1), Rr=(16, 16, 3),
        fp32=dict(tiles=(32, 32, 32, 32), y=(32, 1), yr=(32, 1)),
        fp64=dict(tiles=(32, 32, 32, 8), y=(32, 1), yr=(32, 1)),
        cols=(64, 1), rows4=(4,) * 8 + (1,))),
    "widex": Row((5, 6, 515), SP, 0.7, 2.0, PRECS, 37, 1.0, 9.0, dict(
        Rs=(4, 3, 3), Rr=(10, 8, 7),
        fp32=dict(tiles=(32, 32, 32, 16)),
        fp64=dict(tiles=(32, 32, 32, 8)),
        x=(256, 256, 3), cols=(64,) * 8 + (3,), rows4=(4, 2))),
}
CASES = [(n, p) for n in ROWS for p in ROWS[n].precs]


def row_image(name):
    """Uniform noise of amplitude 100 about a constant 50 (the offset test_gpu_ced.py's images
    have), its amplitude modulated by exp(amp (u_x + u_y + u_z)) with u in [-1/2, 1/2] along each
    axis: the gradient energy, and with it J, varies over the volume by far more than the
    smoothing at the feature scale evens out."""
    row = ROWS[name]
    rng = np.random.default_rng(row.seed)
    u = [np.linspace(-0.5, 0.5, n) if n > 1 else np.zeros(1) for n in row.shape]
    env = np.exp(row.amp * (u[0][:, None, None] + u[1][None, :, None] + u[2][None, None, :]))
    img = 50.0 + 100.0 * env * (rng.uniform(0.0, 1.0, size=row.shape) - 0.5)
    img.setflags(write=False)
    return img


def sym(C):
    """SoA (6, ...) [xx,xy,xz,yy,yz,zz] -> (..., 3, 3)"""
    A = np.empty(C.shape[1:] + (3, 3))
    for c, (a, b) in enumerate(CN.COMP):
        A[..., a, b] = A[..., b, a] = C[c]
    return A


def tensor_from_eig(mu, V, enh, contrast, exponent, alpha=ALPHA):
    """CN.tensor_from_structure after its eigh: (D SoA, lam (3, ...)) from ascending mu, V."""
    lam = CN.eigenvalue_map(mu, ENH[enh], contrast, exponent, alpha)
    T = np.einsum("...ik,...k,...jk->...ij", V, lam, V)
    return np.stack([T[..., a, b] for a, b in CN.COMP]), np.moveaxis(lam, -1, 0)


class RefCache:
    """The rows' images, reference J and its eigen-decomposition: computed once, shared,
    read-only."""

    def __init__(self):
        self._c = {}

    def _get(self, key, make):
        if key not in self._c:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
            self._c[key] = v
        return self._c[key]

    def image(self, name):
        return self._get(("img", name), lambda: row_image(name))

    def J(self, name, rho=None):
        """J_rho of the restatement, SoA (6, z, y, x); rho: another feature scale than the row's."""
        row = ROWS[name]
        return self._get(("J", name, rho), lambda: CN.structure_tensor(
            self.image(name), row.spacing, row.sigma, row.rho if rho is None else rho))

    def eig(self, name):
        return self._get(("eig", name), lambda: tuple(np.linalg.eigh(sym(self.J(name)))))

    def tensor(self, name, enh, exponent=2.0):
        mu, V = self.eig(name)
        return tensor_from_eig(mu, V, enh, ROWS[name].contrast, exponent)


_REFS = RefCache()  # module-wide: the CPU table tests and the GPU tests share it


@pytest.fixture(scope="module")
def refs():
    yield _REFS
    _REFS._c.clear()


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def precision_of(M, prec):
    return {"fp32": M.FP32, "fp64": M.FP64}[prec]


def row_ctx(M, name, prec, **kw):
    row = ROWS[name]
    p = dict(noise_scale=row.sigma, feature_scale=row.rho, contrast=row.contrast, exponent=2.0, alpha=ALPHA,
             precision=precision_of(M, prec))
    p.update(kw)
    return M.CED(row.shape, row.spacing, **p)


# ------------------------------------------------------------ CPU: the table and the reference

@pytest.mark.parametrize("name", list(ROWS))
def test_rows_cross_what_they_claim(name):
    """The restated tile arithmetic gives, for each row and precision, the claimed radii and
    tiles, taps that fit the LDS cap, the claimed LDS requests, and more than one tile with a
    ragged last one along every claimed axis."""
    row = ROWS[name]
    nz, ny, nx = row.shape
    assert nz * ny * nx <= 1_000_000
    cl = row.claim
    assert set(cl) & set(PRECS) == set(row.precs)
    for prec in row.precs:
        p = ced_plan(row.sigma, row.rho, row.spacing, SIZE[prec])
        pc = cl[prec]
        assert p.fits, (prec, p.lds)
        assert (p.Rs, p.Rr) == (cl["Rs"], cl["Rr"])
        assert (p.ZT, p.YT, p.YR, p.ZR) == pc["tiles"], prec
        for axis, n, tile in (("z", nz, p.ZT), ("y", ny, p.YT), ("yr", ny, p.YR), ("zr", nz, p.ZR)):
            if axis in pc:
                assert split(n, tile) == pc[axis] and ragged(pc[axis], tile), (prec, axis)
        for q, want in pc.get("lds", {}).items():
            assert p.lds[("z", "y", "x", "ry", "rz").index(q)] == want, (prec, q)
    if "x" in cl:
        assert split(nx, XROW) == cl["x"] and ragged(cl["x"], XROW)
    assert split(nx, ZCOLS) == cl["cols"] and ragged(cl["cols"], ZCOLS)
    assert split(ny, ZROWS) == cl["rows4"] and ragged(cl["rows4"], ZROWS)


def test_table_covers_every_form():
    """Across the rows: each of ZT, YT and YR halved at least once (in both precisions for ZT and
    YT / YR), ZR in {32, 16, 8, 4}, a radius of 1, an LDS request within 2 KiB of the cap in both
    precisions, at least three x row blocks with a last one narrower than Rr_x, ragged 64-column
    and 4-row blocks, a 1-plane last tile of ced_rz_k, 1-point last tiles along y and x, and
    rho halos longer than the y and z axes."""
    plans = {(n, p): ced_plan(r.sigma, r.rho, r.spacing, SIZE[p]) for n, r in ROWS.items() for p in r.precs}
    for prec in PRECS:
        mine = [pl for (n, p), pl in plans.items() if p == prec]
        assert any(pl.ZT < 32 for pl in mine), prec
        assert any(pl.YT < 32 for pl in mine), prec
        assert any(pl.YR < 32 for pl in mine), prec
        assert any(KVED_LDS - 2048 <= max(pl.lds) <= KVED_LDS for pl in mine), prec
    assert {pl.ZR for pl in plans.values()} == {32, 16, 8, 4}
    # halved tiles that also split their axis raggedly
    assert ROWS["longz"].claim["fp64"]["z"] == (16, 5) and ROWS["longz32"].claim["fp32"]["z"] == (16, 16, 5)
    assert ROWS["longy"].claim["fp64"]["y"] == ROWS["longy"].claim["fp64"]["yr"] == (16, 16, 5)
    assert ROWS["longy32"].claim["fp32"]["y"] == ROWS["longy32"].claim["fp32"]["yr"] == (16, 16, 5)
    assert ROWS["longz"].claim["fp64"]["zr"][-1] == 1 and ROWS["longz32"].claim["fp32"]["zr"][-1] == 1
    assert ROWS["thick"].claim["Rs"][2] == 1  # a radius of 1: three taps
    w = ROWS["widex"]
    assert len(w.claim["x"]) >= 3 and w.claim["x"][-1] < w.claim["Rs"][0] < w.claim["Rr"][0]
    assert all(w.claim["Rr"][q] > w.shape[2 - q] for q in (1, 2))  # y, z: every index clamped
    t = ROWS["thick"].claim
    assert t["cols"][-1] == 1 and t["rows4"][-1] == 1 and t["fp32"]["y"][-1] == 1
    for n, r in ROWS.items():
        assert ragged(r.claim["cols"], ZCOLS) and ragged(r.claim["rows4"], ZROWS), n


def lambda_spread(mu, contrast, exponent=2.0):
    """(lo, hi, share strictly between 0.2 and 0.9) of the mapped eigenvalue that varies -- EED's
    lam_2 and CED's lam_0, both functions of mu_2 - mu_0 -- per enhancement."""
    out = {}
    for enh, col in (("eed", 2), ("ced", 0)):
        lam = CN.eigenvalue_map(mu, ENH[enh], contrast, exponent, ALPHA)[..., col]
        out[enh] = (lam.min(), lam.max(), ((lam > 0.2) & (lam < 0.9)).mean())
    return out


@pytest.mark.parametrize("name", list(ROWS))
def test_row_contrast_spreads_lambda(name, refs):
    """From the reference alone: with the row's contrast the mapped eigenvalue that varies (EED
    lam_2 = 1 - (1 - alpha) h, CED lam_0 = alpha + (1 - alpha) h, h on mu_2 - mu_0) reaches at
    most 0.2 and at least 0.9 over the volume, and lies strictly between at a tenth of the voxels
    or more -- so lambda as a whole does too (EED's lam_0 is 1 and CED's lam_2 is alpha
    everywhere), and not by being 1 or alpha only."""
    mu, _ = refs.eig(name)
    for enh, (lo, hi, mid) in lambda_spread(mu, ROWS[name].contrast).items():
        print(f"{name} {enh}: the varying lambda in [{lo:.4f}, {hi:.4f}], {mid:.3f} of the voxels in (0.2, 0.9)")
        assert lo <= 0.2 and hi >= 0.9, enh
        assert mid >= 0.1, enh


def test_shared_reference_is_ced_numpy():
    """tensor_from_eig on a shared eigh is CN.tensor_from_structure, bit for bit."""
    img = np.random.default_rng(3).normal(50.0, 20.0, size=(7, 8, 9))
    J = CN.structure_tensor(img, (0.7, 1.1, 0.9), 0.6, 1.5)
    mu, V = np.linalg.eigh(sym(J))
    for enh in ENH:
        for m in (1.0, 2.0, 3.0):
            D, lam = tensor_from_eig(mu, V, enh, 4.0, m)
            Dr, lr = CN.tensor_from_structure(J, ENH[enh], 4.0, m, ALPHA)
            assert np.array_equal(D, Dr) and np.array_equal(lam, lr), (enh, m)


# ------------------------------------------------------------ 1. structure tensor on the rows (GPU)

J32_CEILING = 10 * 4.2e-7  # tests/test_gpu_ced.py: 10 x the CPU fp32 emulation figure
D32_CEILING = 1e-3         # the fp32 tensor ceiling of the VED and CED tests
# 4 x the largest figure measured on an MI355X over the rows, the ramps and the fp32 run of
# section 4 (the docstrings of the tests list every figure); the margin covers seed variation
TOL_J32 = 4 * 9.27e-7   # of max|J|: longy32, 485 rho taps along y
TOL_D32 = 4 * 7.31e-6   # absolute, D and lam: longy32 EED (its lam)
TOL64 = 1e-12
TOL_J = {"fp32": TOL_J32, "fp64": TOL64}
TOL_D = {"fp32": TOL_D32, "fp64": TOL64}


def test_fp32_bounds_stay_under_the_ceilings():
    assert TOL_J32 <= J32_CEILING and TOL_D32 <= D32_CEILING


def worst_of(err, name, prec):
    """Where the largest error lies: index (z, y, x) and the tiles of the row's plan."""
    z, y, x = (int(v) for v in np.unravel_index(np.argmax(err), err.shape))
    row = ROWS[name]
    p = ced_plan(row.sigma, row.rho, row.spacing, SIZE[prec])
    return (f"worst at (z, y, x) = ({z}, {y}, {x}) of {row.shape}: ced_z_k tile {z // p.ZT} (+{z % p.ZT} of {p.ZT}), "
            f"ced_rz_k tile {z // p.ZR} (+{z % p.ZR} of {p.ZR}), ced_y_k tile {y // p.YT} (+{y % p.YT} of {p.YT}), "
            f"ced_ry_k tile {y // p.YR} (+{y % p.YR} of {p.YR}), x row block {x // XROW} (+{x % XROW}), "
            f"column block {x // ZCOLS}, 4-row block {y // ZROWS}")


def relmax(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name,prec", CASES)
def test_structure_tensor_matches_restatement_on_rows(M, refs, name, prec):
    """structure_tensor() -- all five passes, ced_rz_k<T, CED_STRUCTURE> -- against the shared
    reference J: fp64 <= 1e-12, fp32 <= TOL_J32 of max|J|.

    Measured on the MI355X, max|J - ref| / max|J|:
      row       fp32      fp64
      seams     1.96e-07  2.8e-16
      longz     2.28e-07  1.5e-16
      longy     6.76e-07  1.0e-15
      longy32   9.27e-07  -
      longz32   7.06e-07  -
      thick     2.61e-07  2.7e-16
      widex     2.55e-07  4.2e-16
    The fp32 figure grows with the number of taps (101 to 485 along the long axis of the long
    rows) and stays under the ceiling of 4.2e-6 with the 4 x margin; none of the worst voxels
    lies on a tile seam.
    """
    v = row_ctx(M, name, prec)
    J = v.structure_tensor(refs.image(name))
    v.close()
    ref = refs.J(name)
    d = np.abs(J - ref).max(axis=0)
    err = d.max() / np.abs(ref).max()
    print(f"structure tensor {name} {prec}: {err:.3e} of max|J| (bound {TOL_J[prec]:.2e}); {worst_of(d, name, prec)}")
    assert err <= TOL_J[prec]


# ------------------------------------------------------------ 2. tensor and lambda on the rows (GPU)

def lam_against_own_tensor(D, lam):
    """max |sorted lam - eigvalsh(D)| over the volume: lam are the eigenvalues of the returned D."""
    return np.abs(np.sort(np.moveaxis(lam, 0, -1), axis=-1) - np.linalg.eigvalsh(sym(D))).max()


@pytest.mark.gpu
@pytest.mark.parametrize("enh", list(ENH))
@pytest.mark.parametrize("name,prec", CASES)
def test_tensor_matches_restatement_on_rows(M, refs, name, prec, enh):
    """tensor(with_lambda=True) -- ced_rz_k<T, CED_TENSOR>: eigen-analysis, eigenvalue map, the six
    components and the three lam volumes -- against the restatement on the shared reference J,
    the maximum over D and lam and the whole volume: fp64 <= 1e-12, fp32 <= TOL_D32 absolute.
    lam against the eigenvalues of the returned D itself: 1e-12 in both precisions (module
    docstring), which a lam volume written with another stride or to another plane misses even
    where its values are plausible.

    Measured on the MI355X, max(|D - ref|, |lam - ref|) EED / CED; lam against eigh(D) is at
    most 2.7e-15 in every case:
      row       fp32                 fp64
      seams     4.61e-06 / 4.47e-06  9.0e-15 / 1.5e-14
      longz     1.61e-06 / 1.89e-06  4.2e-15 / 2.7e-15
      longy     2.61e-06 / 2.96e-06  5.0e-15 / 7.2e-15
      longy32   7.30e-06 / 5.31e-06  -
      longz32   5.20e-06 / 1.87e-06  -
      thick     3.77e-07 / 1.35e-06  2.2e-15 / 7.5e-15
      widex     1.51e-06 / 1.42e-06  4.3e-15 / 3.9e-15
    """
    v = row_ctx(M, name, prec, enhancement=enh)
    D, lam = v.tensor(refs.image(name), with_lambda=True)
    v.close()
    Dr, lr = refs.tensor(name, enh)
    dD, dl = np.abs(D - Dr).max(axis=0), np.abs(lam - lr).max(axis=0)
    own = lam_against_own_tensor(D, lam)
    print(f"tensor {name} {prec} {enh}: max|D - ref| = {dD.max():.3e}, max|lam - ref| = {dl.max():.3e} "
          f"(bound {TOL_D[prec]:.2e}), lam against eigh(D) {own:.3e} (bound 1e-12), "
          f"lam in [{lam.min():.4f}, {lam.max():.4f}]; {worst_of(np.maximum(dD, dl), name, prec)}")
    assert max(dD.max(), dl.max()) <= TOL_D[prec]
    assert own <= 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("exponent", [1.0, 1.5, 3.0])
def test_other_exponents_on_seams(M, refs, exponent):
    """ced_stop's pow with exponents other than 2, fp64 on the seams row, EED and CED: 1e-12
    absolute for D and lam (the 3D counterpart of test_gpu_ced2d.py's test_other_exponents).
    With the row's contrast the varying lambda still spans [0.2, 0.9] at each exponent (asserted).

    Measured on the MI355X, max(|D - ref|, |lam - ref|) EED / CED:
      m = 1.0: 6.0e-15 / 1.1e-14;  m = 1.5: 7.6e-15 / 1.2e-14;  m = 3.0: 1.3e-14 / 2.2e-14
    """
    mu, _ = refs.eig("seams")
    for enh, (lo, hi, _) in lambda_spread(mu, ROWS["seams"].contrast, exponent).items():
        assert lo <= 0.2 and hi >= 0.9, enh
    for enh in ENH:
        v = row_ctx(M, "seams", "fp64", enhancement=enh, exponent=exponent)
        D, lam = v.tensor(refs.image("seams"), with_lambda=True)
        v.close()
        Dr, lr = refs.tensor("seams", enh, exponent)
        err, lerr = np.abs(D - Dr).max(), np.abs(lam - lr).max()
        print(f"tensor seams fp64 {enh} m = {exponent}: max|D - ref| = {err:.3e}, max|lam - ref| = {lerr:.3e} "
              f"(bound 1e-12)")
        assert err <= 1e-12 and lerr <= 1e-12


# ------------------------------------------------------------ 3. designed structure tensors

# u = a . p at the physical points p has the gradient a wherever no tap is clamped (sum K0 = 1,
# sum t K1 = 1), i.e. Rs + Rr or more from every face, so J = a a^T there: eigenvalues
# (0, 0, |a|^2), an exactly repeated pair.  With h = exp(-(K^2 / |a|^2)^m) and n = a / |a|:
#   EED  D = I - (1 - alpha) h n n^T        CED  D = (alpha + (1 - alpha) h) (I - n n^T) + alpha n n^T
# Default spacing, scales, contrast and exponent of M.CED (1, 0.5 / 2.0, 1, 2): Rs = 2, Rr = 8.
RSHAPE = (24, 26, 40)
RHALO = 10  # Rs + Rr
RIN = (slice(RHALO, -RHALO),) * 3
RAMP_CASES = {  # a (x, y, z)
    "x": (1.1, 0.0, 0.0), "y": (0.0, 1.05, 0.0), "z": (0.0, 0.0, 1.15),  # J diagonal: no rotation
    "xy": (0.8, 0.8, 0.0), "xz": (0.75, 0.0, 0.75), "yz": (0.0, 0.78, 0.78),  # 45 degrees, a zero row
    "xyz": (0.6, 0.6, 0.6),
    "generic": (0.7, 0.5, 0.6), "flipped": (0.7, -0.5, 0.6),
}


def ramp_image(case):
    a = RAMP_CASES[case]
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in RSHAPE], indexing="ij")
    return a[0] * x + a[1] * y + a[2] * z


def ramp_analytic(case, enh):
    """(D as six components, h) in the interior, M.CED's default parameters."""
    a = np.array(RAMP_CASES[case])
    a2 = float(a @ a)
    h = np.exp(-(1.0 / a2) ** 2)
    nn = np.outer(a, a) / a2
    if enh == "eed":
        T = np.eye(3) - (1.0 - ALPHA) * h * nn
    else:
        T = (ALPHA + (1.0 - ALPHA) * h) * (np.eye(3) - nn) + ALPHA * nn
    return np.array([T[i, j] for i, j in CN.COMP]), h


class RampRefs:
    """The restatement's (D, lam) of the ramps, shared by the precisions."""

    def __init__(self):
        self._c = {}

    def get(self, case, enh):
        if case not in self._c:
            J = CN.structure_tensor(ramp_image(case), (1.0, 1.0, 1.0), 0.5, 2.0)
            self._c[case] = (J,) + tuple(np.linalg.eigh(sym(J)))
        _, mu, V = self._c[case]
        return tensor_from_eig(mu, V, enh, 1.0, 2.0)

    def J(self, case):
        self.get(case, "eed")
        return self._c[case][0]


_RAMPS = RampRefs()


@pytest.fixture(scope="module")
def ramp_refs():
    yield _RAMPS
    _RAMPS._c.clear()


@pytest.mark.parametrize("case", list(RAMP_CASES))
def test_ramps_have_the_structure_they_claim(case, ramp_refs):
    """From the restatement alone, in the interior: J = a a^T and the tensor is the analytic one,
    both to 1e-12 (measured <= 5e-15 and <= 5e-16), and h lies in [0.2, 0.8] -- a tensor of I or
    alpha I would prove nothing.  The interior is not empty (4 x 6 x 20 voxels)."""
    a = np.array(RAMP_CASES[case])
    Jin = ramp_refs.J(case)[(slice(None),) + RIN]
    assert Jin[0].size == 4 * 6 * 20
    want = np.array([a[i] * a[j] for i, j in CN.COMP])
    eJ = np.abs(Jin - want[:, None, None, None]).max()
    print(f"ramp {case}: interior |J - a a^T| {eJ:.2e}")
    assert eJ <= 1e-12
    for enh in ENH:
        Da, h = ramp_analytic(case, enh)
        assert 0.2 <= h <= 0.8
        D, _ = ramp_refs.get(case, enh)
        eD = np.abs(D[(slice(None),) + RIN] - Da[:, None, None, None]).max()
        print(f"ramp {case} {enh}: h = {h:.3f}, interior |D - analytic| {eD:.2e}")
        assert eD <= 1e-12


@pytest.fixture(scope="module")
def ramp_ctx(M):
    """One context per (precision, enhancement) for all the ramps."""
    made = {}

    def get(prec, enh):
        if (prec, enh) not in made:
            made[(prec, enh)] = M.CED(RSHAPE, precision=precision_of(M, prec), enhancement=enh)
        return made[(prec, enh)]
    yield get
    for v in made.values():
        v.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", list(RAMP_CASES))
def test_eigen_analysis_on_ramps(M, ramp_ctx, ramp_refs, case, prec):
    """sym3_eigen inside ced_point on structure tensors of known eigen-structure (RAMP_CASES: an
    exactly repeated pair everywhere in the interior; already diagonal J, 45-degree rotations
    with a zero row, (1, 1, 1), a generic direction and its mirror image), EED and CED: the whole
    volume against the restatement, the interior against the analytic tensor (fp64 1e-12, fp32
    TOL_D32), and the eigenvalues of the returned D inside [alpha, 1] to the same bound.

    Measured on the MI355X, whole volume against the restatement / interior against the analytic
    tensor, the larger of EED and CED:
      case      fp32                 fp64
      x         1.26e-06 / 7.62e-07  1.3e-15 / 1.1e-15
      y         4.62e-07 / 2.57e-07  1.1e-15 / 3.3e-16
      z         4.18e-07 / 1.20e-07  8.9e-16 / 3.3e-16
      xy        9.19e-07 / 5.20e-07  4.4e-15 / 5.6e-16
      xz        1.29e-06 / 1.11e-07  2.3e-15 / 8.9e-16
      yz        4.20e-07 / 3.52e-07  2.9e-15 / 6.7e-16
      xyz       9.24e-07 / 7.81e-08  2.4e-15 / 8.3e-16
      generic   7.70e-07 / 1.42e-07  2.0e-15 / 7.2e-16
      flipped   5.36e-07 / 8.23e-08  2.2e-15 / 7.2e-16
    (all under the rows' largest fp32 figure, so TOL_D32 comes from the rows)
    """
    u = ramp_image(case)
    tol = TOL_D[prec]
    for enh in ENH:
        D, lam = ramp_ctx(prec, enh).tensor(u, with_lambda=True)
        Dr, lr = ramp_refs.get(case, enh)
        Da, _ = ramp_analytic(case, enh)
        whole = max(np.abs(D - Dr).max(), np.abs(lam - lr).max())
        inner = np.abs(D[(slice(None),) + RIN] - Da[:, None, None, None]).max()
        w = np.linalg.eigvalsh(sym(D))
        print(f"ramp {case} {prec} {enh}: whole volume {whole:.3e}, interior against the analytic tensor "
              f"{inner:.3e} (bound {tol:.2e}); eigenvalues of D in [{w.min():.6f}, {w.max():.6f}]")
        assert whole <= tol
        assert inner <= tol
        assert w.min() >= ALPHA - tol and w.max() <= 1.0 + tol


# ------------------------------------------------------------ 4. the unsupported path and the limit

# ced_rz_k holds ZR + 2 Rr_z planes of six volumes over 64 columns; at the floor ZR = 4 that fits
# 128 KiB up to Rr_z = 19 in fp64 and 40 in fp32
UNSUP64 = dict(shape=ROWS["longz"].shape, spacing=ROWS["longz"].spacing, sigma=ROWS["longz"].sigma, rho=2.4)
UNSUP32 = dict(shape=ROWS["longz"].shape, spacing=(1.0, 1.0, 0.4), sigma=0.7, rho=4.1)


def test_unsupported_cases_are_what_they_claim():
    """The restated plan for the error-path test below: longz at rho = 2.4 has Rr_z = 20, which
    the last pass cannot hold in fp64 even at ZR = 4 (135168 B) and holds in fp32; rho = 4.1 at
    hz = 0.4 has Rr_z = 41, past fp32 too (132096 B); in both only the last pass is over.  The
    largest Rr_z that fits is 19 in fp64 and 40 in fp32, so the fp32-only rows are unsupported in
    fp64."""
    p = ced_plan(UNSUP64["sigma"], UNSUP64["rho"], UNSUP64["spacing"], 8)
    assert p.Rr[2] == 20 and p.ZR == 4 and not p.fits and p.lds[4] == 135168
    assert all(n <= KVED_LDS for n in p.lds[:4])
    assert ced_plan(UNSUP64["sigma"], UNSUP64["rho"], UNSUP64["spacing"], 4).fits
    p = ced_plan(UNSUP32["sigma"], UNSUP32["rho"], UNSUP32["spacing"], 4)
    assert p.Rr[2] == 41 and p.ZR == 4 and not p.fits and p.lds[4] == 132096
    assert all(n <= KVED_LDS for n in p.lds[:4])
    for size, most in ((8, 19), (4, 40)):
        assert (4 + 2 * most) * ZCOLS * COPIES["rz"] * size <= KVED_LDS < (4 + 2 * (most + 1)) * ZCOLS * COPIES["rz"] * size
    for name in ("longy32", "longz32"):
        assert not ced_plan(ROWS[name].sigma, ROWS[name].rho, ROWS[name].spacing, 8).fits


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def expect_unsupported(M, call, what):
    with pytest.raises(M.MadError) as e:
        call()
    print(f"{what}: {e.value}")
    assert e.value.code == M.capi.ERR_UNSUPPORTED
    assert len(str(e.value)) > len("mad error 6: ")


@pytest.mark.gpu
def test_unsupported_scales_raise_and_leave_nothing_behind(M, refs):
    """MAD_ERR_UNSUPPORTED from the host-side check before any launch: structure_tensor, tensor
    and run of an fp64 context whose Rr_z is 20, and of an fp32 context whose Rr_z is 41.  The
    refused contexts close; a fresh context at the row's own scales then returns the bits it
    returned before (J, tensor, lambda, one diffusion step).  The same Rr_z = 20 in fp32 is
    supported and meets the fp32 bounds against the restatement.

    Measured on the MI355X, fp32 at rho = 2.4: J 2.95e-07 of max|J|, D and lam 1.11e-06.
    """
    img = refs.image("longz")
    kw = dict(diffusion_iterations=1)

    def outputs():
        v = row_ctx(M, "longz", "fp64", **kw)
        out = (v.structure_tensor(img),) + v.tensor(img, with_lambda=True) + (v.run(img)[0],)
        v.close()
        return out

    before = outputs()
    for prec, case in (("fp64", UNSUP64), ("fp32", UNSUP32)):
        bad = M.CED(case["shape"], case["spacing"], noise_scale=case["sigma"], feature_scale=case["rho"],
                    precision=precision_of(M, prec), **kw)
        expect_unsupported(M, lambda: bad.structure_tensor(img), f"{prec} structure_tensor")
        expect_unsupported(M, lambda: bad.tensor(img, with_lambda=True), f"{prec} tensor")
        expect_unsupported(M, lambda: bad.run(img), f"{prec} run")
        bad.close()
    after = outputs()
    for what, a, b in zip(("J", "D", "lam", "run"), before, after):
        assert same_bits(a, b), what
    # fp32 storage is the way past the fp64 limit
    ok = row_ctx(M, "longz", "fp32", feature_scale=UNSUP64["rho"])
    J = ok.structure_tensor(img)
    D, lam = ok.tensor(img, with_lambda=True)
    ok.close()
    Jr = refs.J("longz", rho=UNSUP64["rho"])
    Dr, lr = tensor_from_eig(*np.linalg.eigh(sym(Jr)), "eed", ROWS["longz"].contrast, 2.0)
    eJ, eD = relmax(J, Jr), max(np.abs(D - Dr).max(), np.abs(lam - lr).max())
    print(f"fp32 at Rr_z = 20: J {eJ:.3e} of max|J| (bound {TOL_J32:.2e}), D and lam {eD:.3e} (bound {TOL_D32:.2e})")
    assert eJ <= TOL_J32 and eD <= TOL_D32
