"""Structure-tensor diffusion (include/mad_ced.h) checks that need no GPU: the C ABI surface,
the descriptor defaults, and properties of the fp64 numpy restatement (tests/ced_numpy.py)
the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

import ced_numpy as CN
import synth
from conftest import ROOT
from multigridanisotropicdiffusion_amd import _capi as C

SP = (0.8, 1.0, 1.25)


def header_functions():
    src = open(os.path.join(ROOT, "include", "mad_ced.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mad_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_ced_symbol():
    L = C.load()
    names = header_functions()
    assert len(names) == 8
    for n in names:
        assert hasattr(L, n), n


def test_ced_exports_equal_the_header():
    assert sorted(C.CED_EXPORTS) == header_functions()
    assert not set(C.CED_EXPORTS) & set(C.EXPORTS)


def test_desc_defaults():
    d = C.CedDesc()
    assert C.load().mad_ced_desc_init(ctypes.byref(d)) == C.OK
    assert d.abi_version == C.ABI_VERSION
    assert d.enhancement == C.CED_EED and (C.CED_EED, C.CED_CED) == (0, 1)
    assert (d.noise_scale, d.feature_scale, d.contrast, d.exponent, d.alpha) == (0.5, 2.0, 1.0, 2.0, 0.01)
    assert (d.iterations, d.diffusion_iterations) == (1, 5)
    assert d.cycle == C.VCYCLE and d.time_step == 0.1 and d.tolerance == 1e-6
    assert d.diffusion_iterations_per_grid == 2
    assert d.smoother == C.GAUSS_SEIDEL and d.precision == C.PRECISION_AUTO
    assert d.device == -1 and d.verbose == 0 and d.options == 0
    assert list(d.size) == [1, 1, 1] and list(d.spacing) == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("enh,val", [(CN.EED, 1.0), (CN.CED, 0.01)])
def test_constant_image_gives_a_multiple_of_identity(enh, val):
    D, lam = CN.ced_tensor(np.full((9, 10, 11), 37.5), SP, enh, 0.7, 2.0, 5.0, 2.0, 0.01)
    for c, want in enumerate((val, 0.0, 0.0, val, 0.0, val)):
        assert np.abs(D[c] - want).max() < 1e-12, c
    assert np.abs(lam - val).max() < 1e-12


def test_ramp_gradient_is_exact_in_the_interior():
    shape = (12, 13, 30)
    x = np.arange(shape[2], dtype=np.float64)
    img = np.broadcast_to(3.0 * x * SP[0], shape).copy()
    gx, gy, gz = CN.gradient(img, SP, 0.7)
    R = CN.VO.kernel_radius(0.7, SP[0])
    assert np.abs(gx[:, :, R:-R] - 3.0).max() < 1e-12
    assert np.abs(gy).max() < 1e-12 and np.abs(gz).max() < 1e-12


@pytest.mark.parametrize("enh", [CN.EED, CN.CED])
def test_tensor_eigenvalues_lie_in_alpha_one(enh):
    img = 100.0 * synth.image((14, 16, 18), seed=9)
    D, lam = CN.ced_tensor(img, SP, enh, 0.7, 2.0, 5.0, 2.0, 0.01)
    assert lam.min() >= 0.01 - 1e-15 and lam.max() <= 1.0 + 1e-15
    A = np.empty(D.shape[1:] + (3, 3))
    for c, (a, b) in enumerate(CN.COMP):
        A[..., a, b] = A[..., b, a] = D[c]
    w = np.linalg.eigvalsh(A)
    assert w.min() >= 0.01 - 1e-12 and w.max() <= 1.0 + 1e-12
    # the map is not degenerate on this image: both ends of [alpha, 1] are reached
    assert lam.min() < 0.02 and lam.max() > 0.98


@pytest.mark.parametrize("enh", [CN.EED, CN.CED])
def test_axis_permutation_permutes_the_tensor(enh):
    """Image (z, y, x) -> (x, z, y) with the spacing permuted to match: new x = old y,
    new y = old z, new z = old x.  The passes then sum in another order: J moves by a few
    1e-16 relative, which D amplifies by about 90 (a 1e-12 perturbation of J moves D by 9e-11),
    so 1e-10 leaves three orders of margin."""
    img = 100.0 * synth.image((10, 12, 14), seed=9)
    kw = dict(enhancement=enh, noise_scale=0.7, feature_scale=2.0, contrast=5.0, exponent=2.0, alpha=0.01)
    D, _ = CN.ced_tensor(img, SP, **kw)
    perm = (2, 0, 1)  # numpy axes of the new array, taken from the old
    Dp, _ = CN.ced_tensor(np.ascontiguousarray(img.transpose(perm)), (SP[1], SP[2], SP[0]), **kw)
    old = {0: 1, 1: 2, 2: 0}  # new physical axis -> old physical axis (0 = x)
    comp = {ab: c for c, ab in enumerate(CN.COMP)}
    for c, (a, b) in enumerate(CN.COMP):
        oc = comp[tuple(sorted((old[a], old[b])))]
        assert np.abs(Dp[c] - D[oc].transpose(perm)).max() < 1e-10, (a, b)
