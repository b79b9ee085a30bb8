"""Rank-slab kernels against the fp64 oracle on ragged tiles, odd slab offsets, every tensor kind.

tests/test_gpu_tiles.py takes every tiled kernel of one GPU across its tile seams; the tests of the
z-slab decomposition (test_gpu_distributed*.py, test_gpu_coarse.py, test_gpu_refine.py, ...) compare
slabs with the one-rank run only, on volumes whose sizes are all even: every slab offset (Geo::zoff)
is even there, no slab has an odd depth, x and y fit one tile or split evenly, and every tensor is
full.  The rows below (ROWS, checked on the CPU by test_rows_do_what_they_claim from the host
planner) have slabs at odd offsets, both hand-overs to the first replicated level (gathered, where
a slab's depth or offset is odd; the slab view of the coarse level + all-gather otherwise), ragged
x and y tiles, vertex-centred axes, slabs of exactly GHOST planes, and the two-colour sweeps of
diagonal and isotropic tensors.  Ranks are threads of this process (distributed.run_local).

Every comparison is made twice: with the oracle (computed once per row, shared, read-only), and
bit for bit with the one-rank run of the same options (residual norms: 1e-12 relative, the
partial sums re-associate).

Tolerances: those of tests/test_gpu_tiles.py (its docstring), unchanged.  The one-pass
residual + restriction is compared with the oracle in fp64 (1e-12: a residual, then a transfer);
in fp32 it must equal the one-rank residual + restriction pair bit for bit, whose two halves are
compared with the oracle on their own.

Not reachable from the kernel-level entry points: the gathered hand-over's restriction.
mad_restrict answers MAD_ERR_UNSUPPORTED for a slab level above a replicated one (asserted), so
gather_level + restrict_full run inside the V-cycle, FMG and filter-run comparisons only.
"""
import collections

import numpy as np
import pytest

import synth
import test_gpu_tiles as tiles
from test_gpu_tiles import CX, DT, EPS32, IX, SPACING, TX, TY, relmax, split

GHOST = 4             # csrc/mad_kernels.hpp: ghost planes per side of a slab's level arrays
TENSOR_GHOST = 8      # csrc/mad_solver.hip: ghost planes per side of a slab's fp64 tensor
BOUNDARY_PLANES = 8   # csrc/mad_solver.hip: z-depth of the split sweep's boundary chunks
FUSED_BLOCKS = 256    # csrc/mad_solver.hip fused_cfg(): workgroups a whole-slab fused launch aims at

# shape, tensor kind, colours, rank counts, min_slab_voxels (1: coarse levels stay distributed down
# to GHOST planes; 0: the default, which replicates everything below level 0 at these sizes),
# level shapes, distributed levels, the hand-over onto the first replicated level, and per level
# the tile widths the row is there for (x / y: TX x TY smoother tiles, rx: CX restriction tiles of
# that coarse level, vx: the interpolation form onto that level)
Row = collections.namedtuple("Row", "shape tensor ncolors ranks msv levels dist handover cross")
ROWS = {
    # 5-plane slabs at zoff 0, 5, 10, 15; level 1 replicated through the gather
    "odd5": Row((20, 37, 134), "full", 4, (4,), 0, [(20, 37, 134), (10, 19, 67)], [0], "gather", {
        0: dict(x=(64, 64, 6), y=(16, 16, 5), vx=2)}),
    # 13-plane slabs at zoff 0, 13; odd x and y: the scalar interpolation form onto level 0, level 1
    # vertex-centred in x and y, level 2 in z
    "odd13": Row((26, 35, 131), "full", 4, (2,), 0, [(26, 35, 131), (13, 18, 66), (7, 9, 33)], [0],
                 "gather", {0: dict(x=(64, 64, 3), y=(16, 16, 3), vx=1, centering=[0, 0, 1])}),
    # as odd13 with x, y = 1 (mod 4): levels 1 and 2 vertex-centred in x and y, level 2 in z too
    "odd13v": Row((26, 33, 129), "full", 4, (2,), 0, [(26, 33, 129), (13, 17, 65), (7, 9, 33)], [0],
                  "gather", {0: dict(x=(64, 64, 1), y=(16, 16, 1), vx=1, centering=[0, 0, 1])}),
    # levels 0, 1 distributed, level 2 by the even hand-over through two CX tiles; 8 ranks: level-1
    # slabs of GHOST planes; 2 ranks: 32-plane slabs (two z-chunks: split, single-launch, peer forms)
    "deep134": Row((64, 37, 134), "full", 4, (2, 4, 8), 1,
                   [(64, 37, 134), (32, 19, 67), (16, 10, 34)], [0, 1], "even", {
                       0: dict(x=(64, 64, 6), y=(16, 16, 5), vx=2),
                       1: dict(x=(64, 3), y=(16, 3), vx=1),
                       2: dict(rx=(32, 2))}),
    "diag66": Row((32, 40, 66), "diag", 2, (4,), 1, [(32, 40, 66), (16, 20, 33), (8, 10, 17)],
                  [0, 1], "even", {0: dict(x=(64, 2), y=(16, 16, 8), vx=2), 1: dict(vx=1)}),
    "iso129": Row((32, 65, 129), "iso", 2, (2,), 1, [(32, 65, 129), (16, 33, 65), (8, 17, 33)],
                  [0, 1], "even", {0: dict(x=(64, 64, 1), y=(16, 16, 16, 16, 1), vx=1),
                                   1: dict(x=(64, 1), y=(16, 16, 1), vx=1)}),
}
CASES = [(n, p) for n, r in ROWS.items() for p in r.ranks]
CASE_IDS = [f"{n}-{p}ranks" for n, p in CASES]


def plans(name, nranks):
    """[rank][level] -> dict(size, z0, z1, distributed) from the host planner."""
    from multigridanisotropicdiffusion_amd import distributed as D
    row = ROWS[name]
    return [D.plan(row.shape, nranks, r, min_slab_voxels=row.msv) for r in range(nranks)]


def even_handover(fine, coarse, nranks):
    """csrc/mad_solver.hip resid_restrict(), `const bool handover = ...`: level l distributed,
    l + 1 replicated, z cell-centred, and on this rank F.g.nz % 2 == 0 && F.g.zoff % 2 == 0 &&
    (F.g.nz / 2) * nranks == global coarse nz.  Otherwise the descent gathers the fine level."""
    nz, zoff = fine["z1"] - fine["z0"], fine["z0"]
    return (fine["distributed"] and not coarse["distributed"] and fine["size"][2] % 2 == 0 and
            nz % 2 == 0 and zoff % 2 == 0 and (nz // 2) * nranks == coarse["size"][2])


# ------------------------------------------------------------------ the sweep forms
GS, WJ = 0, 2                                   # mad_desc.smoother
OVERLAP, PEER = 2, 4                            # MAD_OPT_OVERLAP_RANK_SWEEP, MAD_OPT_PEER_HALO
Form = collections.namedtuple("Form", "kw single needs")
FORMS = {
    "pc": Form(dict(smoother=GS, gs_kernel=1), "pc", None),
    "pc_peer": Form(dict(smoother=GS, gs_kernel=1, options=PEER), "pc", None),
    "fused": Form(dict(smoother=GS, gs_kernel=3), "fused", None),
    "fused_split": Form(dict(smoother=GS, gs_kernel=3, options=OVERLAP), "fused", "split"),
    "fused_peer": Form(dict(smoother=GS, gs_kernel=3, options=PEER), "fused", "peer"),
    "fused_single": Form(dict(smoother=GS, gs_kernel=4), "fused_single", "single"),
    "wj": Form(dict(smoother=WJ), "wj", None),
}
THIN = "not applicable: slab too thin"


def fused_zc(name, l, fp32, nz):
    """(planes per z-chunk, z-chunks) of a whole-slab fused launch: fused_shape / whole_range."""
    row = ROWS[name]
    ny, nx = row.levels[l][-2:]
    ty = 32 if (row.tensor == "full" and fp32) else 16
    ntiles = len(split(nx, 64)) * len(split(ny, ty))
    chunks = max(1, min((FUSED_BLOCKS + ntiles - 1) // ntiles, max(1, nz // 16)))
    zc = (nz + chunks - 1) // chunks
    return zc, (nz + zc - 1) // zc


def form_runs(name, nranks, form, l, fp32):
    """Does the forced form run as itself on level l's slabs (else the sweep falls back to the
    serial fused launch, which the "fused" form covers)?  Restates sweep_overlap(), peer_eligible()
    and fused_sweep()'s single-launch test of csrc/mad_solver.hip."""
    nz = ROWS[name].levels[l][0] // nranks
    zc, nchunks = fused_zc(name, l, fp32, nz)
    needs = FORMS[form].needs
    if needs == "split":
        return nz >= 3 * BOUNDARY_PLANES
    if needs == "single":
        return nz >= 3 * BOUNDARY_PLANES and nchunks >= 2
    if needs == "peer":
        return nchunks >= 2 and zc >= GHOST
    return form != "pc_peer" or nz >= GHOST


def expected_kernel(name, nranks, form, l, fp32, kname):
    """The form that ran, from smooth_kernel_name(l): a forced form that fell back fails here."""
    runs = form_runs(name, nranks, form, l, fp32)
    tag = {"pc": "gs_color_k<", "pc_peer": "gs_color_k<", "wj": "wj3_k<"}.get(form, "gs_fused3_k<")
    assert kname.startswith(tag), (form, l, kname)
    want = {"split": "boundary + interior launches", "single": "single launch, edge signals",
            "peer": "peer halo, edge planes stored by the sweep"}.get(FORMS[form].needs)
    if form == "pc_peer":
        want = "peer halo, edge planes pushed after the last colour pass"
    if want is not None and runs:
        assert want in kname, (form, l, kname)
    else:
        assert "[rank slab" not in kname, (form, l, kname)


# ------------------------------------------------------------------ CPU: the table itself

@pytest.mark.parametrize("name,nranks", CASES, ids=CASE_IDS)
def test_rows_do_what_they_claim(name, nranks):
    """From the host planner alone: the levels, which of them are distributed, every rank's
    planes, the odd offsets and depths of the odd* rows and that they are what makes
    resid_restrict() refuse the hand-over, the tile splits and the interpolation form."""
    row = ROWS[name]
    pl = plans(name, nranks)
    nl = len(row.levels)
    for r, p in enumerate(pl):
        assert len(p) == nl
        assert [tuple(reversed(q["size"])) for q in p] == row.levels
        assert [l for l, q in enumerate(p) if q["distributed"]] == row.dist
        for l, q in enumerate(p):
            nz = row.levels[l][0]
            if q["distributed"]:
                assert nz % nranks == 0
                assert (q["z0"], q["z1"]) == (r * (nz // nranks), (r + 1) * (nz // nranks)), (r, l)
                assert nz // nranks >= GHOST
            else:
                assert (q["z0"], q["z1"]) == (0, nz), (r, l)
    # without min_slab_voxels = 1 the "deep" rows would keep level 0 only; the odd rows need none
    if row.msv:
        from multigridanisotropicdiffusion_amd import distributed as D
        assert [q["distributed"] for q in D.plan(row.shape, nranks, 0)] == [True] + [False] * (nl - 1)
    ho = row.dist[-1]  # the hand-over: the last distributed level onto the first replicated one
    even = [even_handover(p[ho], p[ho + 1], nranks) for p in pl]
    depth = pl[0][ho]["z1"] - pl[0][ho]["z0"]
    if row.handover == "gather":
        # the gather is taken by every rank (the condition is collective in effect: an odd depth
        # fails it everywhere), and the odd depth alone is what fails it
        assert not any(even)
        assert depth % 2 == 1 and any(p[0]["z0"] % 2 == 1 for p in pl)
        assert row.levels[1][0] * 2 == row.levels[0][0]  # z is cell-centred: not the reason
        assert {"odd5": (5, [0, 5, 10, 15]), "odd13": (13, [0, 13]),
                "odd13v": (13, [0, 13])}[name] == (depth, [p[0]["z0"] for p in pl])
    else:
        assert all(even)
        assert all(p[l]["z0"] % 2 == 0 for p in pl for l in row.dist)

    def ragged(widths, tile):
        return len(widths) > 1 and widths[-1] < tile and all(w == tile for w in widths[:-1])

    for l, claim in row.cross.items():
        nzl, ny, nx = row.levels[l]
        assert nx >= tiles.MIN_TILED and ny >= tiles.MIN_TILED or "x" not in claim
        if "x" in claim:
            assert split(nx, TX) == claim["x"] and ragged(claim["x"], TX), l
        if "y" in claim:
            assert split(ny, TY) == claim["y"] and ragged(claim["y"], TY), l
        if "vx" in claim:
            assert claim["vx"] == (2 if nx % 2 == 0 else 1), (l, nx)
            assert ragged(split(nx, IX * claim["vx"]), IX * claim["vx"]) or nx < IX * claim["vx"], l
        if "rx" in claim:
            assert split(nx, CX) == claim["rx"] and ragged(claim["rx"], CX), l
        if "centering" in claim:  # of level l + 1 w.r.t. l: 1 cell (even size), 0 vertex
            assert [int(n % 2 == 0) for n in reversed(row.levels[l])] == claim["centering"], l
    if name == "deep134":
        d1 = row.levels[1][0] // nranks
        if nranks == 8:  # level-1 slabs of GHOST planes: the tensor's ghost planes span two neighbours
            assert d1 == GHOST and TENSOR_GHOST == 2 * d1
        if nranks == 2:  # two z-chunks per tile column of a whole-slab fused launch, in both precisions
            assert [fused_zc(name, 0, fp32, 32) for fp32 in (True, False)] == [(16, 2), (16, 2)]
    if name == "odd13v":  # levels 1 and 2 vertex-centred in x and y, level 2 in z as well
        assert [n % 2 for n in row.levels[0][1:]] == [1, 1]
        assert [n % 2 for n in row.levels[1]] == [1, 1, 1]


def test_table_covers_every_form():
    """The rows together: an odd zoff, a gathered and an even hand-over, a slab of exactly GHOST
    planes, ragged x and y tiles on a slab, both interpolation forms, every tensor kind; every
    sweep form on a ragged row, and on the odd rows every form a 5- or 13-plane slab can take
    (the split, single-launch and peer forms of the fused sweep need 24 / 32 planes: THIN)."""
    assert {"odd5", "odd13"} <= set(ROWS)
    odd = [n for n, r in ROWS.items() if any(p[0]["z0"] % 2 for P in r.ranks for p in plans(n, P))]
    assert {"odd5", "odd13"} <= set(odd)
    assert {ROWS[n].handover for n in odd} == {"gather"}
    assert any(r.handover == "even" for r in ROWS.values())
    assert {r.tensor for r in ROWS.values() if r.handover == "even"} == {"full", "diag", "iso"}
    depths = {(n, P, l): ROWS[n].levels[l][0] // P for n, P in CASES for l in ROWS[n].dist}
    assert any(d == GHOST and l >= 1 for (n, P, l), d in depths.items())
    assert any(d % 2 == 1 for d in depths.values())
    claims = [(n, l, cl) for n, r in ROWS.items() for l, cl in r.cross.items() if l in r.dist]
    assert any("x" in cl for _, _, cl in claims) and any("y" in cl for _, _, cl in claims)
    assert any("x" in cl and l >= 1 for _, l, cl in claims)
    assert {cl["vx"] for _, _, cl in claims} == {1, 2}
    assert {cl["vx"] for n, _, cl in claims if n in odd} == {1, 2}
    assert any("rx" in cl for r in ROWS.values() for cl in r.cross.values())
    table = {}
    for form in FORMS:
        for n, P in CASES:
            for fp32 in (True, False):
                ls = [l for l in ROWS[n].dist if form_runs(n, P, form, l, fp32)]
                table[form, n, P, fp32] = ls if ls else THIN
    for form in FORMS:
        ragged_rows = {n for (f, n, P, _), v in table.items() if f == form and v != THIN
                       and any("x" in ROWS[n].cross.get(l, {}) for l in v)}
        assert ragged_rows, form
        on_odd = {n for (f, n, P, _), v in table.items() if f == form and v != THIN and n in odd}
        if FORMS[form].needs is None:
            assert {"odd5", "odd13"} <= on_odd, form
        else:
            assert not on_odd, form  # THIN: 5 and 13 planes are under 3 * BOUNDARY_PLANES
            assert max(d for (n, P, l), d in depths.items() if n in odd) < 3 * BOUNDARY_PLANES
    # two colours on more than one rank, on slabs of GHOST planes too
    assert any(ROWS[n].ncolors == 2 and d == GHOST for (n, P, l), d in depths.items())


# ------------------------------------------------------------------ GPU plumbing

class Ctx(tiles.Ctx):
    """tests/test_gpu_tiles.Ctx over this module's rows."""

    def __init__(self, oracle_mod, name):
        row = ROWS[name]
        self.name, self.row, self.om = name, row, oracle_mod
        shape = row.shape
        self.dim = 3
        self.spacing = SPACING
        self.T = {"full": lambda: synth.random_spd(shape, seed=1),
                  "diag": lambda: synth.random_spd(shape, seed=1, offdiag=False),
                  "iso": lambda: synth.isotropic(shape)}[row.tensor]()
        self.o = oracle_mod.Oracle(shape, self.spacing, self.T, DT)
        assert [self.o.shape_at(l) for l in range(self.o.num_levels)] == row.levels
        self._cache = {}

    def _gs3(self, l):  # three sweeps
        x, b = self.get("gs", l), self.get("b", l)
        for _ in range(2):
            x = self.o.gs_color(l, x, b, ncolors=self.row.ncolors)
        return x

    def _rr(self, l):  # R (b - A x)
        return self.o.restrict(l, self.get("residual", l))

    def _interp_x(self, l):  # P x[l + 1]
        return self.o.interpolate(l, self.get("x", l + 1))

    def _ghost_gs(self, l):  # one sweep from 2 P x[l + 1]
        return self.o.gs_color(l, 2.0 * self.get("interp_x", l), self.get("b", l),
                               ncolors=self.row.ncolors)


@pytest.fixture(scope="module")
def ctx_of(oracle_mod):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = Ctx(oracle_mod, name)
        return cache[name]
    yield get
    cache.clear()


@pytest.fixture(scope="module")
def single_runs():
    """One-rank results, shared between the rank counts and the forms that are one on one rank."""
    cache = {}
    yield cache
    cache.clear()


@pytest.fixture(params=["fp32", "fp64"])
def prec(request):
    import multigridanisotropicdiffusion_amd as M
    return M.FP32 if request.param == "fp32" else M.FP64


def run_single(c, body, **kw):
    import multigridanisotropicdiffusion_amd as M
    s = M.Solver(c.row.shape, SPACING, time_step=DT, **kw)
    s.set_tensor(c.T)
    s.setup()
    assert [s.shape_at(l) for l in range(s.num_levels)] == c.row.levels
    out = body(s, [(0, sh[0]) for sh in c.row.levels])
    s.close()
    return out


def run_slabs(c, nranks, body, **kw):
    """body(solver, [(z0, z1) per level]) on every rank; a list of the rank results."""
    from multigridanisotropicdiffusion_amd import distributed as D
    pl = plans(c.name, nranks)

    def rank(r, s):
        s.set_tensor(c.T)
        s.setup()
        for l, q in enumerate(pl[r]):
            assert s.shape_at(l) == (q["z1"] - q["z0"],) + c.row.levels[l][1:], (r, l)
        return body(s, [(q["z0"], q["z1"]) for q in pl[r]])
    return D.run_local(nranks, rank, c.row.shape, spacing=SPACING, time_step=DT,
                       min_slab_voxels=c.row.msv, **kw)


def joined(c, outs, key, l):
    """Level-l arrays of the ranks as one global array (slabs), or every rank's copy (replicated)."""
    if l in c.row.dist:
        return [np.concatenate([o[key] for o in outs])]
    return [o[key] for o in outs]


def check(c, what, outs, one, key, l, ref, tol):
    """Every rank's result against the oracle within tol of max|ref|, and bit for bit against
    the one-rank run."""
    for a in joined(c, outs, key, l):
        e = relmax(a, ref)
        print(f"{c.name} {len(outs)} ranks l={l} {what}: {e:.2e} (bound {tol:.1e})")
        assert e < tol, (what, l)
        np.testing.assert_array_equal(a, one[key], err_msg=f"{what}, level {l}: slabs != one rank")


def check_norms(c, what, outs, one, key):
    for o in outs:
        assert abs(o[key] - one[key]) <= 1e-12 * one[key], (what, o[key], one[key])


# ------------------------------------------------------------------ GPU: sweeps and the residual

def sweep_body(c, levels):
    import multigridanisotropicdiffusion_amd as M

    def body(s, zs):
        out = {}
        for l in levels:
            z0, z1 = zs[l]
            out["name", l] = s.smooth_kernel_name(l)
            s.upload(l, M.capi.X, c.get("x", l)[z0:z1])
            s.upload(l, M.capi.B, c.get("b", l)[z0:z1])
            out["norm", l] = s.residual(l)
            out["r", l] = s.download(l, M.capi.R)
            s.smooth(l, 1)
            out["x", l] = s.download(l, M.capi.X)
            # (also takes in the edge planes a peer form left in flight before the ranks go)
            out["norm1", l] = s.residual(l)
        return out
    return body


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,nranks", CASES, ids=CASE_IDS)
def test_sweep_forms_every_distributed_level(name, nranks, form, prec, ctx_of, single_runs):
    """One sweep of every form on every distributed level -- per-colour passes (with and without
    the pushed peer halo), the fused sweep serial, split (boundary + interior launches), as one
    signalling launch and with the peer halo stored by the sweep, weighted Jacobi -- and residual(l)
    (array and norm) of the same inputs."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)
    row, fp32 = c.row, prec == M.FP32
    f = FORMS[form]
    if f.needs and not any(form_runs(name, nranks, form, l, fp32) for l in row.dist):
        pytest.skip(THIN)
    body = sweep_body(c, row.dist)
    skey = (name, prec, "sweep", f.single)
    if skey not in single_runs:
        single_runs[skey] = run_single(c, body, precision=prec, **{k: v for k, v in f.kw.items()
                                                                  if k != "options"})
    one = single_runs[skey]
    outs = run_slabs(c, nranks, body, precision=prec, **f.kw)
    for l in row.dist:
        for o in outs:
            expected_kernel(name, nranks, form, l, fp32, o["name", l])
        print(f"{name} {nranks} ranks l={l} {form}: {outs[0]['name', l]}")
        if form == "wj":
            check_wj(c, prec, outs, one, l)
        else:
            check(c, form, outs, one, ("x", l), l, c.get("gs", l), 1e-12 if not fp32 else 64 * EPS32)
        check_residual(c, prec, outs, one, l)
        check_norms(c, form, outs, one, ("norm1", l))


def check_wj(c, prec, outs, one, l):
    import multigridanisotropicdiffusion_amd as M
    wj, = joined(c, outs, ("x", l), l)
    ref = c.get("wj", l)
    if prec == M.FP64:
        e = relmax(wj, ref)
        print(f"{c.name} {len(outs)} ranks l={l} wj: {e:.2e} (bound 1e-12)")
        assert e < 1e-12, l
    else:
        mag, dg = c.get("mag_diag", l)
        e = (np.abs(wj - ref) / (mag / dg + np.abs(c.get("x", l)))).max() / EPS32
        print(f"{c.name} {len(outs)} ranks l={l} wj: {e:.2f} eps32 of mag (bound 16)")
        assert e < 16, l
    np.testing.assert_array_equal(wj, one["x", l], err_msg=f"wj, level {l}: slabs != one rank")


def check_residual(c, prec, outs, one, l):
    import multigridanisotropicdiffusion_amd as M
    r, = joined(c, outs, ("r", l), l)
    ref = c.get("residual", l)
    nref = np.linalg.norm(ref)
    for o in outs:
        nrm = o["norm", l]
        if prec == M.FP64:
            en = abs(nrm - nref) / nref
            print(f"{c.name} {len(outs)} ranks l={l} residual norm: {en:.2e} (bound 1e-12)")
            assert en < 1e-12, l
        else:  # the norm of the fp32 residual it belongs to, as tests/test_gpu_tiles.py
            en = abs(nrm - np.linalg.norm(r)) / np.linalg.norm(r)
            print(f"{c.name} {len(outs)} ranks l={l} residual norm: {en:.2e} (bound 1e-6)")
            assert en < 1e-6, l
    if prec == M.FP64:
        e = relmax(r, ref)
        print(f"{c.name} {len(outs)} ranks l={l} residual: {e:.2e} (bound 1e-12)")
        assert e < 1e-12, l
    else:
        mag, _ = c.get("mag_diag", l)
        e = (np.abs(r - ref) / mag).max() / EPS32
        print(f"{c.name} {len(outs)} ranks l={l} residual: {e:.2f} eps32 of mag (bound 16)")
        assert e < 16, l
    np.testing.assert_array_equal(r, one["r", l], err_msg=f"residual, level {l}: slabs != one rank")
    check_norms(c, "residual norm", outs, one, ("norm", l))


# ------------------------------------------------------------------ GPU: transfers

def transfer_body(c, levels):
    import multigridanisotropicdiffusion_amd as M
    X, B, R = M.capi.X, M.capi.B, M.capi.R
    ho = c.row.dist[-1]  # the last distributed level: onto the first replicated one

    def unsupported(call):
        with pytest.raises(M.capi.MadError) as e:
            call()
        return e.value.code == M.capi.ERR_UNSUPPORTED and "replicated level" in str(e.value)

    def body(s, zs):
        out = {}
        slabs = s._desc.nranks > 1
        for l in levels:
            (z0, z1), (c0, c1) = zs[l], zs[l + 1]
            s.upload(l, R, c.get("fine", l)[z0:z1])
            s.upload(l, X, c.get("x", l)[z0:z1])
            s.upload(l, B, c.get("b", l)[z0:z1])
            if slabs and l == ho:
                # mad_restrict of a slab onto the replicated level is refused (the V-cycle gathers
                # there: test_one_vcycle_on_slabs); so is the pair mad_residual_restrict falls back
                # to where the one-pass hand-over does not apply (an odd slab depth or offset)
                out["restrict_refused", l] = unsupported(lambda: s.restrict(l))
                if c.row.handover == "gather":
                    out["rr_refused", l] = unsupported(lambda: s.residual_restrict(l))
            else:
                s.restrict(l)
                out["restrict", l] = s.download(l + 1, B)
                s.residual(l)
                s.restrict(l)
                out["pair", l] = s.download(l + 1, B)
            if not (slabs and l == ho and c.row.handover == "gather"):
                s.upload(l + 1, B, np.full(s.shape_at(l + 1), 7.0))
                out["fused", l] = s.residual_restrict(l)
                out["rr", l] = s.download(l + 1, B)
            s.upload(l + 1, X, c.get("coarse", l)[c0:c1])
            s.interpolate(l)
            out["interp", l] = s.download(l, X)
            s.upload(l, X, c.get("x", l)[z0:z1])
            s.prolongate_add(l)  # x's ghost planes are not current: owned planes only
            out["padd", l] = s.download(l, X)
            # onto the ghost planes too (kbase = -GHOST): written by interpolate(l), added to by
            # prolongate_add(l) now that they are current; the sweep then reads them unexchanged
            s.upload(l + 1, X, c.get("x", l + 1)[c0:c1])
            s.interpolate(l)
            s.prolongate_add(l)
            out["padd2", l] = s.download(l, X)
            s.smooth(l, 1)
            out["ghost_gs", l] = s.download(l, X)
            out["norm", l] = s.residual(l)
        return out
    return body


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("name,nranks", CASES, ids=CASE_IDS)
def test_transfers_across_slab_seams_and_the_handover(name, nranks, prec, ctx_of, single_runs):
    """restrict(l), residual_restrict(l), interpolate(l) and prolongate_add(l) from every
    distributed level: slab to slab (coarse taps and fine ghost planes in global indices, zoff),
    and onto / from the first replicated level.  Onto it, the one-pass even hand-over leaves the
    oracle's whole coarse array on every rank; mad_restrict, and with it mad_residual_restrict
    where a slab's odd depth rules the one-pass form out, answer MAD_ERR_UNSUPPORTED on every rank
    (the gathered descent has no kernel-level entry point: the V-cycle tests run it)."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)
    row, fp64 = c.row, prec == M.FP64
    body = transfer_body(c, row.dist)
    skey = (name, prec, "transfer")
    if skey not in single_runs:
        one = single_runs[skey] = run_single(c, body, precision=prec)
        for l in row.dist:  # one rank: the pair against the oracle, the one-pass form against the pair
            assert one["fused", l]
            np.testing.assert_array_equal(one["rr", l], one["pair", l])
            assert relmax(one["restrict", l], c.get("restrict", l)) < (1e-14 if fp64 else 4 * EPS32), l
    one = single_runs[skey]
    outs = run_slabs(c, nranks, body, precision=prec)
    tol = 1e-14 if fp64 else 4 * EPS32
    gtol = 1e-12 if fp64 else 64 * EPS32
    for l in row.dist:
        ho = l + 1 not in row.dist
        if ho:
            assert all(o["restrict_refused", l] for o in outs), l
            print(f"{name} {nranks} ranks l={l}: restrict onto the replicated level refused "
                  f"(MAD_ERR_UNSUPPORTED) on every rank")
        else:
            check(c, "restrict", outs, one, ("restrict", l), l + 1, c.get("restrict", l), tol)
        if ho and row.handover == "gather":
            assert all(o["rr_refused", l] for o in outs), l
            print(f"{name} {nranks} ranks l={l}: residual_restrict refused (MAD_ERR_UNSUPPORTED) "
                  f"on every rank: no one-pass hand-over from slabs of odd depth")
        else:
            # the one-pass form runs slab to slab and through the even hand-over
            assert all(o["fused", l] for o in outs), l
            if fp64:
                check(c, "residual_restrict", outs, one, ("rr", l), l + 1, c.get("rr", l), 1e-12)
            for a in joined(c, outs, ("rr", l), l + 1):  # = one rank's residual + restriction pair
                np.testing.assert_array_equal(a, one["pair", l], err_msg=f"rr, level {l}: slabs != one rank")
        if not ho:
            if fp64:
                check(c, "residual + restrict", outs, one, ("pair", l), l + 1, c.get("rr", l), 1e-12)
            for a in joined(c, outs, ("pair", l), l + 1):
                np.testing.assert_array_equal(a, one["pair", l], err_msg=f"pair, level {l}: slabs != one rank")
        check(c, "interpolate", outs, one, ("interp", l), l, c.get("interp", l), tol)
        check(c, "prolongate_add", outs, one, ("padd", l), l, c.get("x", l) + c.get("interp", l), tol)
        check(c, "prolongate_add, ghost planes", outs, one, ("padd2", l), l,
              2.0 * c.get("interp_x", l), tol)
        check(c, "sweep on interpolated ghost planes", outs, one, ("ghost_gs", l), l,
              c.get("ghost_gs", l), gtol)
        check_norms(c, "transfers", outs, one, ("norm", l))


# ------------------------------------------------------------------ GPU: cycles

@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("smoother_key", ["gs", "wj"])
@pytest.mark.parametrize("name,nranks", CASES, ids=CASE_IDS)
def test_one_vcycle_on_slabs(name, nranks, smoother_key, prec, ctx_of, single_runs):
    """One V-cycle (nu = 2) with the oracle's smoother and colour order: the descent through the
    hand-over, the replicated levels, the way back up onto the slabs' ghost planes."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)

    def body(s, zs):
        z0, z1 = zs[0]
        s.upload(0, M.capi.X, c.get("x", 0)[z0:z1])
        s.upload(0, M.capi.B, c.get("b", 0)[z0:z1])
        s.vcycle()
        return {"x": s.download(0, M.capi.X), "norm": s.residual(0)}
    kw = dict(precision=prec, smoother=GS if smoother_key == "gs" else WJ)
    skey = (name, prec, "vcycle", smoother_key)
    if skey not in single_runs:
        single_runs[skey] = run_single(c, body, **kw)
    one = single_runs[skey]
    outs = run_slabs(c, nranks, body, **kw)
    check(c, "vcycle " + smoother_key, outs, one, "x", 0, c.get("vcycle_" + smoother_key, 0),
          1e-10 if prec == M.FP64 else 2e-5)
    check_norms(c, "vcycle", outs, one, "norm")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("gs_kernel", [1, 3])
@pytest.mark.parametrize("name,nranks", [(n, p) for n, p in CASES if n in ("odd5", "deep134")],
                         ids=[i for i in CASE_IDS if i.startswith(("odd5", "deep134"))])
def test_three_sweeps_with_b_in_the_records(name, nranks, gs_kernel, prec, ctx_of, single_runs):
    """cycle = SMOOTHER: the level-0 records carry b, on a slab its ghost planes the neighbours'
    (sync_brec); three sweeps, so the second and third start from exchanged planes."""
    import multigridanisotropicdiffusion_amd as M
    c = ctx_of(name)

    def body(s, zs):
        z0, z1 = zs[0]
        name0 = s.smooth_kernel_name(0)
        s.upload(0, M.capi.X, c.get("x", 0)[z0:z1])
        s.upload(0, M.capi.B, c.get("b", 0)[z0:z1])
        s.smooth(0, 3)
        return {"x": s.download(0, M.capi.X), "norm": s.residual(0), "name": name0}
    kw = dict(precision=prec, smoother=GS, gs_kernel=gs_kernel, cycle=M.capi.SMOOTHER)
    skey = (name, prec, "brec", gs_kernel)
    if skey not in single_runs:
        single_runs[skey] = run_single(c, body, **kw)
    one = single_runs[skey]
    outs = run_slabs(c, nranks, body, **kw)
    for o in outs:
        if gs_kernel == 3:  # "... 2, BREC, PEER, BL, ZU, BS>"
            assert o["name"].startswith("gs_fused3_k<") and ", 2, true, " in o["name"], o["name"]
        else:
            assert o["name"].startswith("gs_color_k<"), o["name"]
    print(f"{name} {nranks} ranks: {outs[0]['name']}")
    check(c, f"three sweeps, gs_kernel {gs_kernel}", outs, one, "x", 0, c.get("gs3", 0),
          1e-12 if prec == M.FP64 else 64 * EPS32)
    check_norms(c, "three sweeps", outs, one, "norm")


@pytest.mark.gpu
@pytest.mark.parametrize("name,nranks", [("odd13", 2), ("deep134", 4)])
def test_filter_run_on_odd_and_ragged_slabs_bitwise(name, nranks):
    """Solver.run over two time steps at tolerance 1e-10 (FP32_REFINE: fp64 residual, fp32 cycles),
    each rank passing its slab of an fp32 image: the same cycle counts on every rank as on one
    rank, and the same output bit for bit (tests/test_gpu_distributed.py
    test_filter_run_rank_slabs_bitwise at even shapes)."""
    import multigridanisotropicdiffusion_amd as M
    from multigridanisotropicdiffusion_amd import distributed as D
    row = ROWS[name]
    T = synth.random_spd(row.shape, seed=1)
    img = (synth.image(row.shape, seed=5) * 100).astype(np.float32)
    kw = dict(spacing=SPACING, time_step=DT, tolerance=1e-10, number_of_steps=2)
    s = M.Solver(row.shape, **kw)
    assert s.resolved_precision == M.capi.FP32_REFINE
    s.set_tensor(T)
    ref, rst = s.run(img, out_dtype=np.float64)
    s.close()
    sl = D.slabs(row.shape, nranks)

    def body(r, s):
        s.set_tensor(T)
        s.setup()
        z0, z1 = sl[r]
        return s.run(img[z0:z1], out_dtype=np.float64)
    outs = D.run_local(nranks, body, row.shape, min_slab_voxels=row.msv, **kw)
    print(f"{name} {nranks} ranks: cycles {rst['step_cycles']} relres {rst['last_relres']:.2e}")
    assert rst["total_cycles"] >= 2
    assert all(o[1]["total_cycles"] == rst["total_cycles"] for o in outs)
    assert all(list(o[1]["step_cycles"]) == list(rst["step_cycles"]) for o in outs)
    np.testing.assert_array_equal(np.concatenate([o[0] for o in outs]), ref)
