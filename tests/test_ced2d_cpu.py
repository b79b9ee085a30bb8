"""2D structure-tensor diffusion (include/mad_ced.h, dim = 2) checks that need no GPU: the
descriptor's new field inside the old layout, and properties of the fp64 numpy restatement
(tests/ced2d_numpy.py) the GPU tests compare against."""
import ctypes

import numpy as np
import pytest

import ced2d_numpy as C2
import synth
from multigridanisotropicdiffusion_amd import _capi as C

SP = (0.8, 1.25)
KW = dict(noise_scale=0.7, feature_scale=2.0, contrast=5.0, exponent=2.0, alpha=0.01)


class OldCedDesc(ctypes.Structure):
    """mad_ced_desc before `dim`: int32_t reserved[5] after options."""
    _fields_ = [(n, t) for n, t in C.CedDesc._fields_ if n not in ("dim", "reserved")] + \
               [("reserved", ctypes.c_int32 * 5)]


def test_desc_keeps_its_layout_and_defaults_to_three_dimensions():
    assert ctypes.sizeof(C.CedDesc) == ctypes.sizeof(OldCedDesc)
    for name, _ in OldCedDesc._fields_[:-1]:
        assert getattr(C.CedDesc, name).offset == getattr(OldCedDesc, name).offset, name
    assert C.CedDesc.dim.offset == OldCedDesc.reserved.offset
    assert C.CedDesc.reserved.offset == OldCedDesc.reserved.offset + 4

    # the library's own struct is that size: mad_ced_desc_init clears sizeof(mad_ced_desc)
    # bytes, and the guard bytes behind them stay
    class Guarded(ctypes.Structure):
        _fields_ = [("d", C.CedDesc), ("guard", ctypes.c_uint8 * 16)]
    g = Guarded()
    ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
    assert C.load().mad_ced_desc_init(ctypes.byref(g.d)) == C.OK
    assert g.d.dim == 3 and list(g.d.reserved) == [0, 0, 0, 0]
    assert bytes(g.guard) == b"\xa5" * 16
    assert g.d.options == 0 and g.d.device == -1


def test_stats_keep_their_size():
    class OldCedStats(ctypes.Structure):
        _fields_ = [(n, t) for n, t in C.CedStats._fields_ if n not in ("tile", "reserved")] + \
                   [("reserved", ctypes.c_int32 * 7)]
    assert ctypes.sizeof(C.CedStats) == ctypes.sizeof(OldCedStats)
    assert C.CedStats.stalled.offset == OldCedStats.stalled.offset


def image(shape):
    return 100.0 * synth.image(shape, seed=9)


@pytest.mark.parametrize("enh", [C2.EED, C2.CED])
@pytest.mark.parametrize("shape", [(6, 7), (9, 65), (26, 30)])
def test_eigh_tensor_equals_the_closed_form(shape, enh):
    """Pins the written definition: LAPACK's sum lam_i v_i v_i^T against s I + q [[d, b], [b, -d]]
    (measured <= 1.9e-15 absolute)."""
    J = C2.structure_tensor(image(shape), SP, KW["noise_scale"], KW["feature_scale"])
    args = (enh, KW["contrast"], KW["exponent"], KW["alpha"])
    D, lam = C2.tensor_from_structure(J, *args)
    Dc, lc = C2.closed_form(J, *args)
    err, lerr = np.abs(D - Dc).max(), np.abs(lam - lc).max()
    print(f"eigh vs closed form {shape} enh {enh}: D {err:.3e}, lam {lerr:.3e}")
    assert err <= 1e-12 and lerr <= 1e-12


@pytest.mark.parametrize("enh,val", [(C2.EED, 1.0), (C2.CED, 0.01)])
def test_constant_image_gives_a_multiple_of_identity(enh, val):
    D, lam = C2.ced_tensor(np.full((10, 11), 37.5), SP, enh, **KW)
    for c, want in enumerate((val, 0.0, val)):
        assert np.abs(D[c] - want).max() < 1e-12, c
    assert np.abs(lam - val).max() < 1e-12
    Dc, _ = C2.closed_form(C2.structure_tensor(np.full((10, 11), 37.5), SP, 0.7, 2.0), enh, 5.0, 2.0, 0.01)
    for c, want in enumerate((val, 0.0, val)):
        assert np.abs(Dc[c] - want).max() < 1e-12, c


def test_ramp_gradient_is_exact_in_the_interior():
    shape = (13, 30)
    x = np.arange(shape[1], dtype=np.float64)
    img = np.broadcast_to(3.0 * x * SP[0], shape).copy()
    gx, gy = C2.gradient(img, SP, 0.7)
    R = C2.VO.kernel_radius(0.7, SP[0])
    assert np.abs(gx[:, R:-R] - 3.0).max() < 1e-12
    assert np.abs(gy).max() < 1e-12
    y = np.arange(shape[0], dtype=np.float64)
    img = np.broadcast_to((-2.0 * y * SP[1])[:, None], shape).copy()
    gx, gy = C2.gradient(img, SP, 0.7)
    R = C2.VO.kernel_radius(0.7, SP[1])
    assert np.abs(gy[R:-R] + 2.0).max() < 1e-12
    assert np.abs(gx).max() < 1e-12


@pytest.mark.parametrize("enh", [C2.EED, C2.CED])
def test_tensor_eigenvalues_lie_in_alpha_one(enh):
    """On (26, 30): EED lam in [0.0125, 1], CED in [0.01, 0.9975]."""
    D, lam = C2.ced_tensor(image((26, 30)), SP, enh, **KW)
    print(f"enh {enh}: lam in [{lam.min():.4f}, {lam.max():.4f}]")
    assert lam.min() >= 0.01 - 1e-15 and lam.max() <= 1.0 + 1e-15
    A = np.empty(D.shape[1:] + (2, 2))
    for c, (a, b) in enumerate(C2.COMP):
        A[..., a, b] = A[..., b, a] = D[c]
    w = np.linalg.eigvalsh(A)
    assert w.min() >= 0.01 - 1e-12 and w.max() <= 1.0 + 1e-12
    # the map is not degenerate on this image: both ends of [alpha, 1] are reached
    assert lam.min() < 0.02 and lam.max() > 0.98


@pytest.mark.parametrize("enh", [C2.EED, C2.CED])
def test_transposition_transposes_the_tensor(enh):
    """Image (y, x) -> (x, y) with the spacing swapped: xx <-> yy, xy stays.  The passes then
    sum in another order; <= 1e-10 as the 3D permutation test (measured 4.5e-15)."""
    img = image((26, 30))
    D, _ = C2.ced_tensor(img, SP, enh, **KW)
    Dt, _ = C2.ced_tensor(np.ascontiguousarray(img.T), (SP[1], SP[0]), enh, **KW)
    for c, oc in enumerate((2, 1, 0)):
        err = np.abs(Dt[c] - D[oc].T).max()
        print(f"transpose enh {enh} component {c}: {err:.3e}")
        assert err <= 1e-10, c
