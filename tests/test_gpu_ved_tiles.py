"""VED tensor generation across tile seams, over scales and on designed Hessians.

The per-kernel VED tests of tests/test_gpu_ved.py stop at (22, 26, 30): one z tile, one y tile,
nx below every block width, FIR halos longer than their axes.  The rows below (ROWS, checked
on the CPU by test_rows_cross_what_they_claim) cross the 64-column blocks, the 4-row blocks of
ved_fir_z_k, the 256-wide rows of ved_fir_x_k, the halved z / y tiles that long taps force
(ved_scale's ZT / YT loops), the row chunks of ved_iir_x_k and many blocks of ved_iir_grp_k.
On them the Hessian (both operators, both precisions), the response and the tensor are
compared with oracle/ved_oracle.py; the scale argmax and the reuse of a context are compared
bit for bit with single-scale and fresh contexts; the eigen-analysis of ved_point is steered
with quadratic images whose Hessian is known (QUAD_CASES); GenerateDiffusionTensor's
parameters, the two MAD_ERR_UNSUPPORTED paths and a ragged x partition follow.

The library does not report its VED tiles (nothing in include/mad_ved.h does), so the tile
arithmetic is restated here (fir_plan, KVED_LDS, the chunk of 128 bytes): a change of those
constants in csrc/mad_ved.hpp is NOT noticed by this module -- the rows would silently stop
crossing what they claim.  Whoever changes them updates fir_plan with them.

One oracle Hessian per (row, operator, sigma) is computed once and shared (the oracle fixture);
the response / tensor references are VO.multiscale's update applied to those shared Hessians
(test_shared_hessian_reference_is_ved_oracle pins that to VO.ved_tensor / VO.near_ties).

Tolerances (the project's, tests/test_gpu_ved.py)
  Hessian: fp64 <= 1e-12, fp32 <= 2e-6 of max|H_q| per component.
  fp64 mode: response <= 1e-9, tensor <= 1e-6 absolute.
  fp32 mode: response <= 1e-4, tensor <= 1e-3 outside scale near-ties (VO.near_ties' rule,
    at most 1e-3 of the voxels).
  Bitwise tests have none.
"""
import collections
import threading
import zlib

import numpy as np
import pytest

import synth
import ved_oracle as VO

PRECS = ("fp32", "fp64")
SIZE = {"fp32": 4, "fp64": 8}
HTOL = {"fp32": 2e-6, "fp64": 1e-12}

# csrc/mad_ved.hpp, restated (see the module docstring):
KVED_LDS = 131072      # kVedLds: the dynamic LDS cap of the FIR tiles
ZCOLS, ZROWS = 64, 4   # ved_fir_z_k: a block's columns and rows (also ved_fir_y_k's 64 columns)
XROW = 256             # ved_fir_x_k: points of a row per block
IIR_BYTES = 128        # ved_iir_x_k: a row chunk is one 128-byte line of the storage type
XWAVE, GRP = 64, 256   # ved_iir_x_k: x lines per wave; ved_iir_grp_k: lines per block


def split(n, tile):
    """Widths of the tiles that cover n points."""
    return tuple(min(tile, n - i) for i in range(0, n, tile))


def ragged(widths, tile):
    return len(widths) > 1 and widths[-1] < tile and all(w == tile for w in widths[:-1])


def fir_plan(sigma, spacing, size):
    """ved_taps' radius and ved_scale's tile choice for spacing (x, y, z) and a storage type
    of `size` bytes: (R (x, y, z), ZT, YT, whether all three passes fit the LDS cap)."""
    R = tuple(max(1, int(np.ceil(4.0 * sigma / h))) for h in spacing)

    def lds(lines, width, copies):
        return lines * width * copies * size

    ZT = YT = 32
    while ZT > 4 and lds(ZT + 2 * R[2], 256, 1) > KVED_LDS:
        ZT //= 2
    while YT > 4 and lds(YT + 2 * R[1], 64, 3) > KVED_LDS:
        YT //= 2
    need = max(lds(ZT + 2 * R[2], 256, 1), lds(YT + 2 * R[1], 64, 3), lds(256 + 2 * R[0], 1, 6))
    return R, ZT, YT, need <= KVED_LDS


# shape (z, y, x), spacing (x, y, z).  claim: at sigma = 2.0 the taps R (x, y, z) and, per
# precision, ZT / YT with the z / y tile widths (named only where the axis has several tiles)
# and the x chunks of the recursive x pass; x: ved_fir_x_k's rows; cols: the 64-column blocks
# of the z and y passes; rows4: ved_fir_z_k's 4-row blocks; xlines / zlines: the recursive
# passes' x lines per wave and z lines per block.
Row = collections.namedtuple("Row", "shape spacing sigmas precs seed claim")
SP = (0.3125, 0.29, 0.4)
ROWS = {
    "seams": Row((37, 35, 300), SP, (0.6, 2.0), PRECS, 21, dict(
        R=(26, 28, 20),
        fp64=dict(ZT=16, YT=16, z=(16, 16, 5), y=(16, 16, 3), chunks=(16,) * 18 + (12,)),
        fp32=dict(ZT=32, YT=32, z=(32, 5), y=(32, 3), chunks=(32,) * 9 + (12,)),
        x=(256, 44), cols=(64,) * 4 + (44,), rows4=(4,) * 8 + (3,),
        xlines=(64,) * 20 + (15,), zlines=(256,) * 41 + (4,))),
    "one_over": Row((33, 65, 257), SP, (2.0,), PRECS, 22, dict(
        R=(26, 28, 20),
        fp64=dict(ZT=16, YT=16, z=(16, 16, 1), y=(16,) * 4 + (1,), chunks=(16,) * 16 + (1,)),
        fp32=dict(ZT=32, YT=32, z=(32, 1), y=(32, 32, 1), chunks=(32,) * 8 + (1,)),
        x=(256, 1), cols=(64,) * 4 + (1,), rows4=(4,) * 16 + (1,))),
    "deep_z64": Row((37, 9, 70), (0.3125, 0.29, 0.32), (2.0,), ("fp64",), 23, dict(
        R=(26, 28, 25),
        fp64=dict(ZT=8, YT=16, z=(8, 8, 8, 8, 5), chunks=(16,) * 4 + (6,)),
        cols=(64, 6), rows4=(4, 4, 1))),
    "deep_z32": Row((37, 9, 70), (0.3125, 0.29, 0.16), (2.0,), ("fp32",), 24, dict(
        R=(26, 28, 50),
        fp32=dict(ZT=16, YT=32, z=(16, 16, 5), chunks=(32, 32, 6)),
        cols=(64, 6), rows4=(4, 4, 1))),
}
TENSOR_ROWS = {"seams": (0.6, 2.0), "one_over": (2.0,)}  # section 2: the scales per row
OMEGA = 1.5


def row_image(name):
    row = ROWS[name]
    img = np.random.default_rng(row.seed).normal(50.0, 20.0, size=row.shape)
    img.setflags(write=False)
    return img


# ------------------------------------------------------ the reference on shared Hessians

def eig_scale(H, alpha=0.5, beta=0.5, gamma=5.0):
    """One scale's candidates from its oracle Hessian (..., 6): the body of VO.multiscale's
    loop -- (vesselness, eigenvector columns in numpy.linalg.eigh's ascending order)."""
    A = np.empty(H.shape[:-1] + (3, 3))
    A[..., 0, 0], A[..., 0, 1], A[..., 0, 2] = H[..., 0], H[..., 1], H[..., 2]
    A[..., 1, 0], A[..., 1, 1], A[..., 1, 2] = H[..., 1], H[..., 3], H[..., 4]
    A[..., 2, 0], A[..., 2, 1], A[..., 2, 2] = H[..., 2], H[..., 4], H[..., 5]
    w, v = np.linalg.eigh(A)
    return VO.vesselness(VO.sort_by_magnitude(w), alpha, beta, gamma), v


def keep_largest(cands):
    """VO.multiscale's update over the scales' candidates: the first scale unconditionally,
    later ones on a strict > (VED.hxx:272).  Returns (response, Q, index of the kept scale)."""
    resp, Q = cands[0]
    win = np.zeros(resp.shape, np.int64)
    for i, (ves, v) in enumerate(cands[1:], 1):
        upd = ves > resp
        resp = np.where(upd, ves, resp)
        Q = np.where(upd[..., None, None], v, Q)
        win = np.where(upd, i, win)
    return resp, Q, win


def ties_of(cands, rel=1e-6):
    """VO.near_ties' rule on the scales' candidates (no ties with one scale)."""
    if len(cands) < 2:
        return np.zeros(cands[0][0].shape, bool)
    ves = np.sort(np.stack([c[0] for c in cands]), axis=0)
    return (ves[-1] > 0) & ((ves[-1] - ves[-2]) <= rel * ves[-1])


class OracleCache:
    """Oracle Hessians, candidates and tensors of the rows: computed once, shared, read-only."""

    def __init__(self):
        self._c = {}

    def _get(self, key, make):
        if key not in self._c:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._c[key] = v
        return self._c[key]

    def image(self, name):
        return self._get(("img", name), lambda: row_image(name))

    def hessian(self, name, kind, sigma):
        """(z, y, x, 6)"""
        return self._get(("H", name, kind, sigma),
                         lambda: VO.hessian(self.image(name), ROWS[name].spacing, sigma, kind))

    def cands(self, name, kind, scales):
        return [self._get(("cand", name, kind, s), lambda s=s: eig_scale(self.hessian(name, kind, s)))
                for s in scales]

    def tensor(self, name, kind, scales):
        """(tensor (6, z, y, x), response, near-ties, kept scale) at omega = OMEGA, the other
        parameters VED's defaults."""
        def make():
            cands = self.cands(name, kind, scales)
            resp, Q, win = keep_largest(cands)
            return VO.diffusion_tensor(resp, Q, 0.01, OMEGA, 10.0), resp, ties_of(cands), win
        return self._get(("T", name, kind, tuple(scales)), make)


@pytest.fixture(scope="module")
def oracle():
    c = OracleCache()
    yield c
    c._c.clear()


@pytest.fixture(scope="module")
def M():
    import multigridanisotropicdiffusion_amd as mod
    return mod


def precision_of(M, prec):
    return {"fp32": M.FP32, "fp64": M.FP64}[prec]


# ------------------------------------------------------------ CPU: the table and the reference

@pytest.mark.parametrize("name", list(ROWS))
def test_rows_cross_what_they_claim(name):
    """The restated tile arithmetic gives, for each row and precision, the claimed taps, ZT and
    YT, more than one tile with a ragged last one along every claimed axis, and taps that fit
    the LDS cap at every sigma the row runs."""
    row = ROWS[name]
    nz, ny, nx = row.shape
    cl = row.claim
    for prec in row.precs:
        for sigma in row.sigmas:
            assert fir_plan(sigma, row.spacing, SIZE[prec])[3], (prec, sigma)
        R, ZT, YT, _ = fir_plan(2.0, row.spacing, SIZE[prec])
        pc = cl[prec]
        assert R == cl["R"]
        assert (ZT, YT) == (pc["ZT"], pc["YT"]), prec
        assert split(nz, ZT) == pc["z"] and ragged(pc["z"], ZT), prec
        if "y" in pc:
            assert split(ny, YT) == pc["y"] and ragged(pc["y"], YT), prec
        chunk = IIR_BYTES // SIZE[prec]
        assert split(nx, chunk) == pc["chunks"] and ragged(pc["chunks"], chunk), prec
    if "x" in cl:
        assert split(nx, XROW) == cl["x"] and ragged(cl["x"], XROW)
    assert split(nx, ZCOLS) == cl["cols"] and ragged(cl["cols"], ZCOLS)
    assert split(ny, ZROWS) == cl["rows4"] and ragged(cl["rows4"], ZROWS)
    if "xlines" in cl:
        assert split(ny * nz, XWAVE) == cl["xlines"] and ragged(cl["xlines"], XWAVE)
        assert split(nx * ny, GRP) == cl["zlines"] and ragged(cl["zlines"], GRP)


def test_table_covers_every_form():
    """Across the rows, by name: a halved z tile, a halved y tile, a twice-halved z tile, the
    fp32 halved z tile, an x seam, a 1-element last tile on each axis in both precisions, and
    recursive x rows ending in a 1-point chunk in both precisions."""
    claims = {(n, p): r.claim[p] for n, r in ROWS.items() for p in r.precs}
    assert claims[("seams", "fp64")]["ZT"] == 16                     # halved z
    assert claims[("seams", "fp64")]["YT"] == 16 and "y" in claims[("seams", "fp64")]  # halved y
    assert claims[("deep_z64", "fp64")]["ZT"] == 8                   # twice-halved z
    assert claims[("deep_z32", "fp32")]["ZT"] == 16                  # fp32's halved z
    assert claims[("seams", "fp32")]["ZT"] == claims[("seams", "fp32")]["YT"] == 32  # and whole tiles
    assert len(ROWS["seams"].claim["x"]) > 1                         # x seam
    for p in PRECS:
        c = claims[("one_over", p)]
        assert c["z"][-1] == 1 and c["y"][-1] == 1 and c["chunks"][-1] == 1, p
    assert ROWS["one_over"].claim["x"][-1] == 1 and ROWS["one_over"].claim["cols"][-1] == 1
    assert ROWS["one_over"].claim["rows4"][-1] == 1
    # every precision a row runs has a claim, and nothing else
    for n, r in ROWS.items():
        assert set(r.claim) & set(PRECS) == set(r.precs), n


def test_shared_hessian_reference_is_ved_oracle():
    """eig_scale / keep_largest / ties_of on shared Hessians are VO.ved_tensor and VO.near_ties,
    bit for bit (both operators; several scales and one)."""
    rng = np.random.default_rng(3)
    img = rng.normal(50.0, 20.0, size=(9, 10, 12))
    sp = (0.7, 1.1, 0.9)
    for kind in ("recursive", "fir"):
        for scales in ((0.6, 1.0, 2.0), (1.0,)):
            cands = [eig_scale(VO.hessian(img, sp, s, kind)) for s in scales]
            resp, Q, win = keep_largest(cands)
            T = VO.diffusion_tensor(resp, Q, 0.01, OMEGA, 10.0)
            Tr, rr = VO.ved_tensor(img, sp, scales=scales, omega=OMEGA, kind=kind)
            assert np.array_equal(resp, rr) and np.array_equal(T, Tr), (kind, scales)
            ves = np.stack([c[0] for c in cands])
            assert np.array_equal(resp, np.take_along_axis(ves, win[None], axis=0)[0])
            if kind == "recursive" and len(scales) > 1:
                assert np.array_equal(ties_of(cands), VO.near_ties(img, sp, scales, 0.5, 0.5, 5.0))
    assert not ties_of(cands).any()  # one scale


@pytest.mark.parametrize("kind", ["fir", "recursive"])
def test_seams_row_exercises_the_argmax(kind):
    """From the oracle: on the seams image each of the two scales is the kept one at more than
    5 % of the voxels (measured: FIR 20 % / 10 %, recursive 20 % / 10 %; 70 % of the voxels
    have zero response), so a wrong scale selection moves the tensor where it is looked at."""
    img = row_image("seams")
    cands = [eig_scale(VO.hessian(img, ROWS["seams"].spacing, s, kind)) for s in TENSOR_ROWS["seams"]]
    resp, _, win = keep_largest(cands)
    share = [((win == i) & (resp > 0)).mean() for i in range(2)]
    print(f"seams {kind}: scale wins {share[0]:.3f} / {share[1]:.3f}, zero response {(resp == 0).mean():.3f}")
    assert min(share) > 0.05


# ------------------------------------------------------------ 1. Hessian on the rows (GPU)

HESS_CASES = [(n, k, p) for n in ROWS for k in ("fir", "recursive") for p in ROWS[n].precs]


def worst_of(err, name, prec):
    """Where the largest error lies: index (z, y, x) and the tiles of the row's plan."""
    z, y, x = (int(v) for v in np.unravel_index(np.argmax(err), err.shape))
    _, ZT, YT, _ = fir_plan(2.0, ROWS[name].spacing, SIZE[prec])
    chunk = IIR_BYTES // SIZE[prec]
    return (f"worst at (z, y, x) = ({z}, {y}, {x}): z tile {z // ZT} (+{z % ZT} of {ZT}), y tile {y // YT} "
            f"(+{y % YT} of {YT}), x row block {x // XROW} (+{x % XROW}), column block {x // ZCOLS}, "
            f"4-row block {y // ZROWS}, x chunk {x // chunk} (+{x % chunk} of {chunk})")


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,prec", HESS_CASES)
def test_hessian_matches_oracle_on_rows(M, oracle, name, kind, prec):
    """ComputeHessian at every sigma of the row against the oracle, per component, at the
    project's bounds (fp64 1e-12, fp32 2e-6 of max|H_q|).

    Measured on the MI355X (largest component error over the row's sigmas):
      row        FIR fp64  FIR fp32  recursive fp64  recursive fp32
      seams      4.6e-15   5.9e-07   0 (bitwise)     4.2e-07
      one_over   3.2e-15   6.3e-07   0               3.3e-07
      deep_z64   3.7e-15   -         0               -
      deep_z32   -         5.5e-07   -               3.8e-07
    Before ved_fir_z_k took the image's offset off in the fp32 mode (ved_offset_k) the FIR fp32
    xx component missed the bound on three rows: seams 3.09e-06, one_over 2.38e-06, deep_z32
    2.63e-06, each far from any tile seam.  A numpy restatement of the fp32 sums gave the same
    figures to three digits: rounding of eps32 |image| (mean 50, deviation 20) through 53 taps
    that cancel, not a tile error; (22, 26, 30) of test_gpu_ved.py sits at 1.5e-06 for the same
    reason and has 20 times fewer voxels to draw its maximum from.
    """
    row = ROWS[name]
    img = oracle.image(name)
    v = M.VED(row.shape, row.spacing, precision=precision_of(M, prec), hessian=kind)
    bad = []
    for sigma in row.sigmas:
        H = v.hessian(img, sigma)
        ref = oracle.hessian(name, kind, sigma)
        errs = []
        for q in range(6):
            d = np.abs(H[q] - ref[..., q])
            e = d.max() / np.abs(ref[..., q]).max()
            errs.append(e)
            if not e < HTOL[prec]:
                bad.append((sigma, q, e, worst_of(d, name, prec)))
        print(f"{name} {kind} {prec} sigma={sigma}: max|H_q - ref| / max|ref_q| = "
              + " ".join(f"{e:.2e}" for e in errs) + f" (bound {HTOL[prec]:.0e})")
    v.close()
    for b in bad:
        print("  over the bound: sigma=%g component %d: %.3e, %s" % b)
    assert not bad, [b[:3] for b in bad]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name", list(ROWS))
def test_recursive_passes_are_bitwise_the_line_walk_on_rows(M, oracle, name, prec):
    """test_gpu_ved.py's bitwise test carried to the rows: ved_iir_x_k over many chunks (the last
    one of 12, 6 or 1 point), 1295 / 2145 x lines off the 64-line wave, thousands of z and y
    lines over many 256-line blocks of ved_iir_grp_k equal ved_iir_k's one thread per line."""
    row = ROWS[name]
    img = oracle.image(name)
    H = {}
    for opt in (0, M.capi.VED_OPT_LINE_WALK):
        v = M.VED(row.shape, row.spacing, precision=precision_of(M, prec), options=opt)
        H[opt] = [v.hessian(img, s) for s in row.sigmas]
        v.close()
    for s, a, b in zip(row.sigmas, H[0], H[M.capi.VED_OPT_LINE_WALK]):
        ndiff = int((a != b).sum())
        print(f"{name} {prec} sigma={s}: {ndiff} of {a.size} values differ from the line walk")
        assert ndiff == 0, (s, worst_of(np.abs(a - b).max(axis=0), name, prec))


# ------------------------------------------------------------ 2. response and tensor on the rows

@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["fir", "recursive"])
@pytest.mark.parametrize("name", list(TENSOR_ROWS))
def test_tensor_matches_oracle_on_rows(M, oracle, name, kind, prec):
    """v.tensor() on the multi-tile rows (seams: two scales, the argmax exercised; one_over: one
    scale) at omega = 1.5.  fp64: response 1e-9, tensor 1e-6.  fp32: response 1e-4, tensor 1e-3
    outside the scale near-ties, which are fewer than 1e-3 of the voxels.

    Measured on the MI355X (response / tensor error); the near-tie share is exactly 0 on both
    rows and operators:
      row       operator   fp64               fp32
      seams     FIR        1.3e-15 / 5.5e-13  1.8e-07 / 3.9e-05
      seams     recursive  4.4e-16 / 3.6e-14  2.5e-07 / 7.1e-05
      one_over  FIR        4.5e-16 / 3.0e-13  4.0e-08 / 1.2e-05
      one_over  recursive  9.5e-17 / 8.1e-14  5.4e-08 / 4.5e-05
    (one_over FIR fp32 had a response error of 2.2e-04, over the bound, before ved_offset_k:
    see test_hessian_matches_oracle_on_rows.)
    """
    row = ROWS[name]
    scales = TENSOR_ROWS[name]
    Tr, rr, tie, _ = oracle.tensor(name, kind, scales)
    v = M.VED(row.shape, row.spacing, omega=OMEGA, scales=scales, precision=precision_of(M, prec),
              hessian=kind)
    T, resp = v.tensor(oracle.image(name))
    v.close()
    er = np.abs(resp - rr).max()
    dT = np.abs(T - Tr).max(axis=0)
    if prec == "fp64":
        print(f"{name} {kind} fp64: response {er:.2e} (bound 1e-9), tensor {dT.max():.2e} (bound 1e-6)")
        assert er < 1e-9
        assert ((resp > 0) == (rr > 0)).mean() > 0.999
        assert dT.max() < 1e-6, worst_of(dT, name, prec)
    else:
        out = np.where(tie, 0.0, dT)
        print(f"{name} {kind} fp32: response {er:.2e} (bound 1e-4), tensor outside near-ties {out.max():.2e} "
              f"(bound 1e-3), everywhere {dT.max():.2e}, near-tie share {tie.mean():.2e} (bound 1e-3)")
        assert er < 1e-4
        assert tie.mean() < 1e-3
        assert not (out > 1e-3).any(), worst_of(out, name, prec)


# ------------------------------------------------------------ 3. scale argmax and reuse, bitwise

def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["fir", "recursive"])
def test_scale_argmax_composes_bitwise(M, oracle, kind, prec):
    """UpdateVesselness over two scales is the composition of the single-scale runs: the response
    is their maximum and the tensor that of the first scale attaining it (the strict > of
    VED.hxx:272), bit for bit; with the scales reversed the response is the same and the
    tensor too wherever the two responses differ.  Same kernels on both sides: no tolerance."""
    row = ROWS["seams"]
    img = oracle.image("seams")
    scales = TENSOR_ROWS["seams"]

    def run(sc):
        v = M.VED(row.shape, row.spacing, omega=OMEGA, scales=sc, precision=precision_of(M, prec), hessian=kind)
        out = v.tensor(img)
        v.close()
        return out

    (T0, r0), (T1, r1) = run(scales[:1]), run(scales[1:])
    T, r = run(scales)
    Tb, rb = run(scales[::-1])
    later = r1 > r0
    print(f"seams {kind} {prec}: later scale kept at {later.mean():.3f}, first at {((r0 >= r1) & (r0 > 0)).mean():.3f}, "
          f"equal nonzero responses at {((r0 == r1) & (r0 > 0)).sum()} voxels")
    assert later.mean() > 0.05 and ((r0 >= r1) & (r0 > 0)).mean() > 0.05
    assert same_bits(r, np.maximum(r0, r1))
    assert same_bits(T, np.where(later[None], T1, T0))
    assert same_bits(rb, r)
    differ = r0 != r1
    assert same_bits(Tb[:, differ], T[:, differ])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kind", ["fir", "recursive"])
def test_context_reuse_is_bitwise(M, oracle, kind, prec):
    """tensor(A), tensor(B), tensor(A) on one context: the third equals the first and the second
    a fresh context's tensor(B); hessian(B) in between changes nothing either.  The first scale
    overwrites resp / dir unconditionally (the `first` flag), whatever an earlier image or a
    Hessian call left in resp, dir and the pass volumes."""
    row = ROWS["seams"]
    A = oracle.image("seams")
    B = np.random.default_rng(77).normal(120.0, 45.0, size=row.shape)
    kw = dict(omega=OMEGA, scales=TENSOR_ROWS["seams"], precision=precision_of(M, prec), hessian=kind)
    v = M.VED(row.shape, row.spacing, **kw)
    TA, rA = v.tensor(A)
    TB, rB = v.tensor(B)
    TA2, rA2 = v.tensor(A)
    v.hessian(B, 2.0)
    TA3, rA3 = v.tensor(A)
    v.close()
    f = M.VED(row.shape, row.spacing, **kw)
    TBf, rBf = f.tensor(B)
    f.close()
    assert not np.array_equal(rA, rB) and (rA > rB).mean() > 0.05 and (rB > rA).mean() > 0.05
    assert same_bits(rA2, rA) and same_bits(TA2, TA)
    assert same_bits(rB, rBf) and same_bits(TB, TBf)
    assert same_bits(rA3, rA) and same_bits(TA3, TA)


# ------------------------------------------------------------ 4. eigen-analysis on designed Hessians

# f(p) = 1/2 p^T A p + b^T p + c at the physical points p has the scale-normalised FIR Hessian
# sigma^2 A wherever the taps are unclamped (the taps are exact on polynomials of degree <= 2).
# A = 2 Q diag(mu) Q^T, so sigma^2 A = 4.5 Q diag(mu) Q^T at sigma = 1.5: the eigenvalues are
# 4.5 mu and the kept direction (largest algebraic eigenvalue) is Q's first column.
QSHAPE, QSP, QSIGMA = (24, 26, 40), (0.8, 1.0, 1.25), 1.5
QR = (8, 6, 5)  # taps (x, y, z)
INTERIOR = (slice(QR[2], -QR[2]), slice(QR[1], -QR[1]), slice(QR[0], -QR[0]))
NROT = 32
QUAD_CASES = {
    "generic": (-0.05, -1.0, -1.3),
    "tube": (0.0, -1.0, -1.0),          # exact double lower pair: the closed form's acos at +-1
    "toppair": (-3.0, -1.0005, -1.0),   # top pair 2.25e-3 apart: sym3_eigvec_closed declines
    "tube_x": (0.0, -1.0, -1.3), "tube_y": (0.0, -1.0, -1.3), "tube_z": (0.0, -1.0, -1.3),
}
AXIS = {"tube_x": 0, "tube_y": 1, "tube_z": 2}


def quad_rotation(case, k):
    """Q of rotation k: a seeded random rotation, or for tube_* the permutation that puts mu_0
    along the axis (two of them: the other two axes in either order)."""
    if case in AXIS:
        a = AXIS[case]
        o = [q for q in range(3) if q != a]
        if k % 2:
            o.reverse()
        Q = np.zeros((3, 3))
        Q[a, 0], Q[o[0], 1], Q[o[1], 2] = 1.0, 1.0, 1.0
        return Q
    rng = np.random.default_rng(zlib.crc32(f"quad/{case}/{k}".encode()))
    Q, Rm = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(Rm))
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    return Q


def quad_nrot(case):
    return 2 if case in AXIS else NROT


def quad_image(case, k):
    """(image (z, y, x), sigma^2 A as a 3x3 matrix in (x, y, z) order)."""
    Q = quad_rotation(case, k)
    A = 2.0 * (Q * np.array(QUAD_CASES[case])) @ Q.T
    A = 0.5 * (A + A.T)
    rng = np.random.default_rng(zlib.crc32(f"quad-b/{case}/{k}".encode()))
    b = rng.normal(0.0, 2.0, size=3)
    nz, ny, nx = QSHAPE
    px = (np.arange(nx) - 0.5 * (nx - 1)) * QSP[0]
    py = (np.arange(ny) - 0.5 * (ny - 1)) * QSP[1]
    pz = (np.arange(nz) - 0.5 * (nz - 1)) * QSP[2]
    Z, Y, X = np.meshgrid(pz, py, px, indexing="ij")
    f = (0.5 * (A[0, 0] * X * X + A[1, 1] * Y * Y + A[2, 2] * Z * Z)
         + A[0, 1] * X * Y + A[0, 2] * X * Z + A[1, 2] * Y * Z + b[0] * X + b[1] * Y + b[2] * Z + 50.0)
    return f, QSIGMA * QSIGMA * A


def sym(H):
    """(..., 6) or (6, ...)-last [xx,xy,xz,yy,yz,zz] -> (..., 3, 3)"""
    A = np.empty(H.shape[:-1] + (3, 3))
    for c, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        A[..., i, j] = A[..., j, i] = H[..., c]
    return A


def closed_form_spread(A):
    """sym3_eigvals_closed's spread = sqrt(p2 / 6), restated."""
    q = np.trace(A) / 3.0
    B = A - q * np.eye(3)
    p1 = A[0, 1] ** 2 + A[0, 2] ** 2 + A[1, 2] ** 2
    p2 = B[0, 0] ** 2 + B[1, 1] ** 2 + B[2, 2] ** 2 + 2.0 * p1
    return np.sqrt(p2 / 6.0)


@pytest.mark.parametrize("case", list(QUAD_CASES))
def test_designed_hessians_have_the_structure_they_claim(case):
    """From the oracle alone, on the interior: the FIR Hessian of the quadratic image is
    sigma^2 A to rounding (|f| <= ~2e3, 17-tap sums: 1e-10 absolute is generous; measured
    <= 2e-13), its eigenvalues are 4.5 mu, and
    generic: all gaps above 0.2;  tube: the lower pair a double to 1e-10, the top one 4.5 away;
    tube_x/y/z: a diagonal Hessian with the top eigenvector the axis;
    toppair: the top gap 2.25e-3 lies below 1e-3 of the restated spread (3.0e-3), with a margin
    (7.5e-4) far above an fp32 Hessian's error (2e-6 of 13.5), so sym3_eigvec_closed declines in
    the fp32 mode at every interior voxel."""
    mu = np.array(QUAD_CASES[case])
    worst = 0.0
    for k in range(quad_nrot(case)):
        f, S = quad_image(case, k)
        H = sym(VO.hessian(f, QSP, QSIGMA, "fir")[INTERIOR])
        worst = max(worst, np.abs(H - S).max())
        assert np.abs(H - S).max() < 1e-10
        w = np.linalg.eigvalsh(H)
        assert np.abs(w - np.sort(QSIGMA ** 2 * 2.0 * mu)).max() < 1e-9
        top, mid, low = w[..., 2], w[..., 1], w[..., 0]
        if case == "generic":
            assert (top - mid).min() > 0.2 and (mid - low).min() > 0.2
        elif case == "tube":
            assert (mid - low).max() < 1e-10 and (top - mid).min() > 4.4
        elif case == "toppair":
            spread = closed_form_spread(S)
            gap = top - mid
            assert 2.2e-3 < gap.min() and gap.max() < 2.3e-3
            assert 2.9e-3 < 1e-3 * spread < 3.1e-3
            assert 1e-3 * spread - gap.max() > 7e-4 > 20 * 2e-6 * np.abs(w).max()
        else:
            a = AXIS[case]
            off = H - H * np.eye(3)
            assert np.abs(off).max() < 1e-10
            assert np.abs(np.linalg.eigh(H)[1][..., a, 2]).min() > 1 - 1e-12
    print(f"{case}: interior |H - sigma^2 A| <= {worst:.2e}")


class QuadOracle:
    """Oracle (tensor, response) of the designed images, shared by the precisions."""

    def __init__(self):
        self._c = {}

    def get(self, case, k, kind):
        key = (case, k, kind)
        if key not in self._c:
            f, _ = quad_image(case, k)
            self._c[key] = VO.ved_tensor(f, QSP, scales=(QSIGMA,), omega=OMEGA, kind=kind)
        return self._c[key]


@pytest.fixture(scope="module")
def quad_oracle():
    c = QuadOracle()
    yield c
    c._c.clear()


@pytest.fixture(scope="module")
def quad_ctx(M):
    """One context per (operator, precision) for all the designed images."""
    made = {}

    def get(kind, prec):
        if (kind, prec) not in made:
            made[(kind, prec)] = M.VED(QSHAPE, QSP, omega=OMEGA, scales=(QSIGMA,), hessian=kind,
                                       precision=precision_of(M, prec))
        return made[(kind, prec)]
    yield get
    for v in made.values():
        v.close()


def projector(T, resp):
    """GenerateDiffusionTensor undone: T = a I + (c - a) d d^T with V = resp^(1/10),
    a = 1 + (eps - 1) V, c = 1 + (omega - 1) V gives P = d d^T, (..., 3, 3)."""
    V = np.power(resp, 1.0 / 10.0)
    a = 1.0 + (0.01 - 1.0) * V
    c = 1.0 + (OMEGA - 1.0) * V
    P = sym(np.moveaxis(T, 0, -1))
    return (P - a[..., None, None] * np.eye(3)) / (c - a)[..., None, None]


def backward_error(H, d):
    """rho = ||H d - (d^T H d) d|| / ||H||_2 per voxel."""
    Hd = np.einsum("...ij,...j->...i", H, d)
    r = Hd - np.einsum("...i,...i->...", d, Hd)[..., None] * d
    return np.linalg.norm(r, axis=-1) / np.abs(np.linalg.eigvalsh(H)).max(axis=-1)


QUAD_GPU = ([(c, "fir") for c in QUAD_CASES] + [("generic", "recursive"), ("tube", "recursive")])
# 4 x the largest rho measured on the MI355X (1.12e-07), far under the 2e-5 above which the bound
# would no longer tell an eigenvector from the plane; see test_eigen_analysis_on_designed_hessians
TOPPAIR_RHO32 = 4.5e-7
TOPPAIR_RHO64 = 1e-12


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case,kind", QUAD_GPU)
def test_eigen_analysis_on_designed_hessians(M, quad_ctx, quad_oracle, case, kind, prec):
    """ved_point on Hessians of known eigen-structure (QUAD_CASES; 32 rotations per case on one
    context per precision, interior voxels): response and tensor against the oracle at the
    project's bars (fp64 1e-9 / 1e-6, fp32 1e-4 / 1e-3); tube_x/y/z also pin the component
    order: the tensor's omega direction is the axis to 1e-6.

    toppair, fp32 (the Jacobi fallback with hardware reciprocals): the direction is ill-conditioned
    against the oracle (rounding the image to fp32 moves the oracle's tensor by 4e-4), so the
    tensor is checked by backward error on the GPU's own fp32 Hessian H: P = d d^T recovered from
    the tensor has trace 1 to 1e-6, and its top eigenvector d has
    rho = ||H d - (d^T H d) d|| / ||H||_2 <= TOPPAIR_RHO32; any vector of the top pair's plane
    reaches 8e-5 .. 1.7e-4, so the bound tells an eigenvector from the plane.  fp64: rho <= 1e-12.
    rho is as small for the pair's other eigenvector, so the Rayleigh quotient is checked too:
    a d with rho under the bound lies within 3e-3 rad of one of the two eigenvectors, i.e.
    (lambda_max - d^T H d) / gap is below 1e-5 or above 1 - 1e-5; it must be below 1/2.

    Measured on the MI355X (32 rotations, interior voxels):
      toppair fp32: rho 1.12e-07 (TOPPAIR_RHO32 = 4 x that, under the ceiling 2e-5), the oracle's
        eigenvector on the same fp32 H: rho 1.36e-06; |tr P - 1| 4.4e-07; response error 2.0e-06;
        tensor against the oracle 7.0e-03 (not asserted: ill-conditioned, above)
      toppair fp64: rho 6.5e-16, the oracle's 3.1e-15; |tr P - 1| 1.6e-15; tensor error 1.2e-11
      generic / tube, FIR: response / tensor 2.4e-06 / 2.8e-06 and 2.0e-06 / 2.7e-06 in fp32,
        <= 5e-15 in fp64; recursive: <= 8.5e-07 in fp32, <= 4e-15 in fp64
      tube_x / y / z: |P - e e^T| 7.5e-07 / 8.6e-07 / 1.9e-07 in fp32, <= 1.2e-15 in fp64
    """
    v = quad_ctx(kind, prec)
    rtol, ttol = (1e-9, 1e-6) if prec == "fp64" else (1e-4, 1e-3)
    er = et = ea = etr = rho = rho_ref = ray = 0.0
    rmin, rmax = np.inf, 0.0
    for k in range(quad_nrot(case)):
        f, _ = quad_image(case, k)
        T, resp = v.tensor(f)
        Tr, rr = quad_oracle.get(case, k, kind)
        T, resp, Tr, rr = T[(slice(None),) + INTERIOR], resp[INTERIOR], Tr[(slice(None),) + INTERIOR], rr[INTERIOR]
        rmin, rmax = min(rmin, rr.min()), max(rmax, rr.max())
        er = max(er, np.abs(resp - rr).max())
        et = max(et, np.abs(T - Tr).max())
        if case in AXIS:
            e = np.zeros((3, 3))
            e[AXIS[case], AXIS[case]] = 1.0
            ea = max(ea, np.abs(projector(T, resp) - e).max())
        if case == "toppair" and kind == "fir":
            H = sym(np.moveaxis(v.hessian(f, QSIGMA), 0, -1)[INTERIOR])
            P = projector(T, resp)
            etr = max(etr, np.abs(np.trace(P, axis1=-2, axis2=-1) - 1.0).max())
            d = np.linalg.eigh(P)[1][..., 2]
            rho = max(rho, backward_error(H, d).max())
            w = np.linalg.eigvalsh(H)
            ray = max(ray, ((w[..., 2] - np.einsum("...i,...ij,...j->...", d, H, d)) / (w[..., 2] - w[..., 1])).max())
            Pr = projector(Tr, rr)
            rho_ref = max(rho_ref, backward_error(H, np.linalg.eigh(Pr)[1][..., 2]).max())
    print(f"{case} {kind} {prec}: interior response in [{rmin:.4f}, {rmax:.4f}], response error {er:.2e} "
          f"(bound {rtol:.0e}), tensor error {et:.2e} (bound {ttol:.0e})")
    assert rmin > 0.05  # the designed Hessians have a response: the tensor carries a direction
    assert er < rtol
    if case in AXIS:
        print(f"{case} {kind} {prec}: |P - e e^T| {ea:.2e} (bound 1e-6)")
        assert ea <= 1e-6
    if case == "toppair" and kind == "fir":
        bound = TOPPAIR_RHO64 if prec == "fp64" else TOPPAIR_RHO32
        print(f"toppair {prec}: |tr P - 1| {etr:.2e} (bound 1e-6), rho {rho:.2e} (bound {bound:.1e}), "
              f"the oracle's eigenvector on the same H: rho {rho_ref:.2e}; "
              f"(lambda_max - d^T H d) / gap {ray:.2e} (bound 0.5)")
        assert etr <= 1e-6
        assert rho <= bound
        assert ray < 0.5
        if prec == "fp32":
            return  # the tensor against the oracle is ill-conditioned here (docstring)
    assert et < ttol


# ------------------------------------------------------------ 5. tensor parameters

PSHAPE = (12, 14, 70)
PARAM_SETS = [dict(epsilon=0.01, omega=5.0, sensitivity=10.0),
              dict(epsilon=0.2, omega=1.5, sensitivity=1.0),
              dict(epsilon=0.5, omega=25.0, sensitivity=4.0),
              dict(epsilon=0.2, omega=1.5, sensitivity=1.0, alpha=0.3, beta=0.8, gamma=20.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("params", PARAM_SETS, ids=lambda p: "-".join(f"{k[0]}{v:g}" for k, v in p.items()))
def test_tensor_parameters_match_oracle(M, params):
    """GenerateDiffusionTensor's epsilon / omega / sensitivity and the vesselness' alpha / beta /
    gamma away from their defaults, fp64, on a crop of the tube phantom (70 columns: two blocks):
    response 1e-9, tensor 1e-6, and voxels with zero response exactly the identity."""
    # the phantom places its tubes 8 voxels inside a volume: a crop of a larger one
    img = synth.tube_phantom((18, 18, 70), seed=4).astype(np.float64)[3:15, 2:16, :]
    assert img.shape == PSHAPE
    sp, scales = (1.0, 0.9, 1.2), (1.0, 2.0)
    v = M.VED(PSHAPE, sp, scales=scales, precision=M.FP64, **params)
    T, resp = v.tensor(img)
    v.close()
    p = dict(alpha=0.5, beta=0.5, gamma=5.0)
    p.update(params)
    Tr, rr = VO.ved_tensor(img, sp, scales=scales, **p)
    zero = resp == 0
    print(f"{params}: response {np.abs(resp - rr).max():.2e} (bound 1e-9), tensor {np.abs(T - Tr).max():.2e} "
          f"(bound 1e-6), zero response at {zero.mean():.3f} of the voxels (oracle {(rr == 0).mean():.3f})")
    assert 0.05 < (rr == 0).mean() < 0.95
    assert np.abs(resp - rr).max() < 1e-9
    assert ((resp > 0) == (rr > 0)).mean() > 0.999
    assert np.abs(T - Tr).max() < 1e-6
    ident = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])
    assert (T[:, zero] == ident[:, None]).all()


# ------------------------------------------------------------ 6. error paths, ragged partition

def test_error_case_taps_exceed_the_lds_cap_in_fp64_only():
    """The restated plan for the error-path test below: spacing 0.25 along z at sigma 2 gives
    R_z = 32, which no fp64 z tile fits (ZT = 4: 139264 B) and fp32 does."""
    R, ZT, _, fits = fir_plan(2.0, (1.0, 1.0, 0.25), 8)
    assert R[2] == 32 and ZT == 4 and not fits
    assert (ZT + 2 * R[2]) * 256 * 8 == 139264
    assert fir_plan(2.0, (1.0, 1.0, 0.25), 4)[3]
    assert fir_plan(0.5, (1.0, 1.0, 0.25), 8)[3]


@pytest.mark.gpu
def test_unsupported_calls_raise_and_leave_the_context_usable(M):
    """MAD_ERR_UNSUPPORTED, no kernel run: FIR taps too long for the LDS tiles (fp64, R_z = 32) and
    the recursive operator on an axis under 4 points.  The FIR context then answers a call with a
    smaller sigma, within the fp64 bound."""
    rng = np.random.default_rng(31)
    shape, sp = (9, 10, 12), (1.0, 1.0, 0.25)
    img = rng.normal(50.0, 20.0, size=shape)
    v = M.VED(shape, sp, precision=M.FP64, hessian="fir")
    with pytest.raises(M.MadError) as ei:
        v.hessian(img, 2.0)
    print("fir:", ei.value)
    assert ei.value.code == M.capi.ERR_UNSUPPORTED
    assert str(ei.value).split(":", 1)[1].strip()
    H = v.hessian(img, 0.5)
    ref = VO.hessian(img, sp, 0.5, "fir")
    e = max(np.abs(H[q] - ref[..., q]).max() / np.abs(ref[..., q]).max() for q in range(6))
    print(f"fir, sigma 0.5 after the refused call: {e:.2e} (bound 1e-12)")
    assert e < 1e-12
    v.close()
    small = (3, 8, 8)
    r = M.VED(small, (1.0, 1.0, 1.0), precision=M.FP64)
    with pytest.raises(M.MadError) as ei:
        r.hessian(rng.normal(50.0, 20.0, size=small), 1.0)
    print("recursive:", ei.value)
    assert ei.value.code == M.capi.ERR_UNSUPPORTED
    assert str(ei.value).split(":", 1)[1].strip()
    r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nranks,xranges", [((32, 20, 37), 4, (9, 9, 9, 10))])
def test_ved_on_ragged_x_partition_matches_single(M, shape, nranks, xranges):
    """test_ved_on_rank_slabs_matches_single's scheme where the ranks' x ranges differ (xr() of
    ved_scale_iir: 37 columns over 4 ranks = 9, 9, 9, 10): transposed blocks of unequal widths;
    the concatenated slabs equal the single-rank output bit for bit."""
    nx = shape[2]
    assert tuple(nx * (r + 1) // nranks - nx * r // nranks for r in range(nranks)) == xranges
    assert len(set(xranges)) > 1
    rng = np.random.default_rng(5)
    img = (rng.normal(100.0, 20.0, size=shape)).astype(np.float32)
    kw = dict(omega=1.5, iterations=2, diffusion_iterations=2, tolerance=1e-6, scales=(0.5, 1.0, 2.0))
    ref, rst = M.VED(shape, (1.0, 1.0, 1.0), **kw).run(img, out_dtype=np.float64)
    outs, errs = [None] * nranks, []
    key = zlib.crc32(repr(("ved-ragged", shape, nranks)).encode())

    def worker(r):
        try:
            v = M.VED(shape, (1.0, 1.0, 1.0), nranks=nranks, rank=r, **kw)
            v.comm_init_local(key)
            outs[r] = v.run(img, out_dtype=np.float64)
            v.close()
        except BaseException as e:  # noqa: BLE001 - reported below
            errs.append((r, e))

    th = [threading.Thread(target=worker, args=(r,)) for r in range(nranks)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    full = np.concatenate([o[0] for o in outs])
    assert full.shape == shape
    assert all(o[1]["total_cycles"] == rst["total_cycles"] for o in outs)
    np.testing.assert_array_equal(full, ref)
