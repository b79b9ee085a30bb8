"""Perona-Malik contrast from a gradient quantile (include/mad_pm.h "Contrast from a quantile",
include/mad_pm_quantile.h) checks that need no GPU: the restatement's rank rule, its K -> 0
limit and its scale covariance, the C ABI layout against the host compiler, and the parameter
validation (mad_pm_create validates before it touches a device)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pm_numpy as P
import pm_quantile_numpy as Q
import synth
from conftest import ROOT
from multigridanisotropicdiffusion_amd import _capi as C
from test_pm_cpu import raw_create

SP2, SP3 = (0.8, 1.25), (0.8, 1.0, 1.25)
KINDS = [P.WEICKERT, P.EXPONENTIAL, P.RATIONAL]


def test_rank_rule_is_numpys_inverted_cdf():
    """On arrays with ties, q in {1 / N, 0.5, 0.9, 1.0} and a few more; the rank's edges."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 10, 100, 1001):
        a = rng.integers(0, max(2, n // 3), size=n).astype(np.float64) / 7.0  # many ties
        for q in (1.0 / n, 0.5, 0.9, 1.0, 0.1, 0.999):
            want = np.quantile(a, q, method="inverted_cdf")
            assert Q.quantile_s(a, q) == want, (n, q)
            assert np.sort(a)[Q.rank(q, n)] == want
    assert Q.rank(1.0, 10) == 9 and Q.rank(0.1, 10) == 0 and Q.rank(0.11, 10) == 1
    assert Q.rank(1e-9, 10) == 0 and Q.rank(0.5, 1) == 0 and Q.rank(0.9, 10) == 8


@pytest.mark.parametrize("kind", KINDS)
def test_zero_contrast_limit(kind):
    """K = 0: g is alpha away from flat voxels and alpha + (1 - alpha) on them, no NaN."""
    alpha = 0.01
    s = np.array([0.0, 5e-324, 1e-300, 1.0, 1e300])
    g = Q.diffusivity_k2(s, kind, 0.0, 2.0, alpha)
    assert not np.isnan(g).any()
    assert g[0] == alpha + (1.0 - alpha) and abs(g[0] - 1.0) <= 2.3e-16
    assert (g[1:] == alpha).all()
    # A constant image and one whose left 95 % is constant both select s_q = 0 at q = 0.9.  The
    # constant is 0: a sum of taps times 0 is exactly 0 in any order, while for another constant c
    # the derivative taps cancel only up to rounding and leave s ~ (1e-16 c)^2, the same bits at
    # every pixel (measured for c = 3: K = 2.2e-17).
    for img in (np.zeros((9, 40)), np.where(np.arange(40) >= 38, 50.0, 0.0) * np.ones((9, 1))):
        D, g, K = Q.pm_tensor(img, (1.0, 1.0), kind, 0.5, 0.9)
        assert K == 0.0 and not np.isnan(D).any()
        assert set(np.unique(g)) <= {alpha, alpha + (1.0 - alpha)}
    assert (Q.pm_tensor(np.zeros((9, 40)), (1.0, 1.0), kind, 0.5, 0.9)[1] == alpha + (1.0 - alpha)).all()
    # any constant: s, hence g, is one value everywhere, in [alpha, 1], and K is 0 or that residue
    _, g, K = Q.pm_tensor(np.full((9, 40), 3.0), (1.0, 1.0), kind, 0.5, 0.9)
    assert len(np.unique(g)) == 1 and alpha <= g.flat[0] <= 1.0 and 0.0 <= K <= 1e-12 * 3.0


def test_map_on_k2_agrees_with_pm_numpy():
    """The restated map takes K^2 itself; with K^2 = K K it is pm_numpy's map."""
    s = np.concatenate([[0.0], np.logspace(-6, 6, 200)])
    for kind in KINDS:
        for m in (1.0, 1.5, 2.0):
            a = Q.diffusivity_k2(s, kind, 3.5 * 3.5, m, 0.02)
            b = P.diffusivity(s, kind, 3.5, m, 0.02)
            assert np.abs(a - b).max() <= 1e-15, (kind, m)


@pytest.mark.parametrize("shape,sp", [((20, 33), SP2), ((7, 9, 12), SP3)])
@pytest.mark.parametrize("kind", KINDS)
def test_scale_covariance_of_the_restatement(shape, sp, kind):
    """u and 4 u: every product of the gradient scales by a power of two, so s scales by exactly
    16, K by exactly 4, and g is the same bits.  A fixed contrast does not have the property."""
    u = 100.0 * synth.image(shape, seed=9)
    _, g1, K1 = Q.pm_tensor(u, sp, kind, 1.0, 0.9)
    _, g4, K4 = Q.pm_tensor(4.0 * u, sp, kind, 1.0, 0.9)
    assert K1 > 0.0 and K4 == 4.0 * K1
    assert g1.tobytes() == g4.tobytes()
    assert g1.min() < 0.5 < g1.max()
    assert P.pm_tensor(u, sp, kind, 1.0, K1)[1].tobytes() != P.pm_tensor(4.0 * u, sp, kind, 1.0, K1)[1].tobytes()


def c_sizes(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mad_pm_quantile.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mad_pm_desc), sizeof(mad_pm_stats), '
                   'offsetof(mad_pm_desc, contrast_mode), offsetof(mad_pm_desc, reserved), '
                   'offsetof(mad_pm_stats, contrast_used), offsetof(mad_pm_stats, reserved)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    return [int(t) for t in subprocess.check_output([exe], text=True).split()]


def test_struct_layout_equals_the_c_compilers(tmp_path):
    """The header as C11 (its _Static_assert included), and the ctypes mirror field by field.
    The sizes are those of the layout before the mode existed: 176 and 88 bytes."""
    desc, stats, o_mode, o_res, o_used, o_sres = c_sizes(tmp_path)
    assert (desc, stats) == (176, 88)
    assert ctypes.sizeof(C.PmDesc) == desc and ctypes.sizeof(C.PmStats) == stats
    assert C.PmDesc.contrast_mode.offset == C.PmDesc.reserved.offset == o_mode == C.PmDesc.dim.offset + 4
    assert o_res == o_mode + 4
    assert C.PmStats.contrast_used.offset == o_used == 72
    assert C.PmStats.reserved.offset == o_sres == 80 and len(C.PmStats().reserved) == 2
    # the binding's four-word `reserved` view starts at the mode: word 0 is contrast_mode
    d = C.PmDesc()
    d.contrast_mode = 1
    assert list(d.reserved) == [1, 0, 0, 0]


def test_quantile_header_and_exports():
    src = open(os.path.join(ROOT, "include", "mad_pm_quantile.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(mad_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(C.PM_QUANTILE_EXPORTS) == ["mad_pm_contrast", "mad_pm_select"]
    L = C.load()
    for n in names:
        assert hasattr(L, n), n
    assert not set(C.PM_QUANTILE_EXPORTS) & (set(C.PM_EXPORTS) | set(C.EXPORTS) | set(C.CED_EXPORTS))
    assert (C.PM_CONTRAST_ABSOLUTE, C.PM_CONTRAST_QUANTILE) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "mad_pm.h")).read()
    assert re.search(r"MAD_PM_CONTRAST_ABSOLUTE = 0,", hdr) and re.search(r"MAD_PM_CONTRAST_QUANTILE = 1\b", hdr)
    assert f"0x{C.PM_OPT_TEST_CONTRAST_IS_SQUARED:08x}u" in hdr.lower()


def test_desc_init_selects_absolute_mode():
    d = C.PmDesc()
    ctypes.memset(ctypes.byref(d), 0xA5, ctypes.sizeof(d))
    assert C.load().mad_pm_desc_init(ctypes.byref(d)) == C.OK
    assert d.contrast_mode == C.PM_CONTRAST_ABSOLUTE and d.options == 0


@pytest.mark.parametrize("bad", [dict(contrast_mode=1, contrast=0.0), dict(contrast_mode=1, contrast=1.5),
                                 dict(contrast_mode=1, contrast=-0.5), dict(contrast_mode=2),
                                 dict(contrast_mode=-1),
                                 dict(contrast_mode=1, contrast=0.9, options=C.PM_OPT_TEST_CONTRAST_IS_SQUARED),
                                 dict(options=C.PM_OPT_TEST_CONTRAST_IS_SQUARED | 1),
                                 # N = 2^32: the selection counts in 32 bits
                                 dict(contrast_mode=1, contrast=0.9, size=(65536, 65536, 1)),
                                 dict(contrast_mode=1, contrast=0.9, size=(2 ** 31, 2, 1)),
                                 dict(contrast_mode=1, contrast=0.9, size=(2 ** 40, 2 ** 40, 2 ** 40))])
def test_invalid_quantile_parameters(bad):
    with pytest.raises(C.MadError) as e:
        raw_create(**bad)
    assert e.value.code == C.ERR_INVALID
    assert len(str(e.value)) > len("mad error 1: ")


def test_python_surface():
    from multigridanisotropicdiffusion_amd import pm
    f = pm.PeronaMalikDiffusionImageFilter()
    assert f.GetContrastUsed() is None and f._p["contrast_quantile"] is None
    f.SetContrastQuantile(0.9)
    assert f._p["contrast_quantile"] == 0.9
    f.SetContrast(4.0)  # back to absolute mode
    assert f._p["contrast_quantile"] is None and f._p["contrast"] == 4.0
    f.SetContrastQuantile(0.5)
    f.SetConductanceParameter(3.0)  # the alias does the same
    assert f._p["contrast_quantile"] is None and f._p["contrast"] == 3.0
    with pytest.raises(ValueError):
        pm.PM2D((9, 10), SP2, contrast_quantile=0.9, _contrast_squared=4.0)
    with pytest.raises(C.MadError) as e:
        pm.PM2D((9, 10), SP2, contrast_quantile=0.0)
    assert e.value.code == C.ERR_INVALID
