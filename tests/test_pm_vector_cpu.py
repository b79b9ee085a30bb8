"""Vector-valued Perona-Malik diffusion (include/mad_pm.h, "Vector-valued images") checks that need
no GPU: the descriptor word, parameter validation (mad_pm_create validates before it touches a
device), the Python contexts' shape checks, and the fp64 restatement (tests/pm_vector_numpy.py)
with the C oracle on the case the feature exists for -- a weak edge in one channel that a strong
edge in another channel protects."""
import ctypes

import numpy as np
import pytest

import pm_numpy as P
import pm_vector_numpy as V
import synth
from multigridanisotropicdiffusion_amd import _capi as C

SP2 = (0.8, 1.25)


def test_desc_init_leaves_channels_zero():
    d = C.PmDesc()
    ctypes.memset(ctypes.byref(d), 0xA5, ctypes.sizeof(d))
    assert C.load().mad_pm_desc_init(ctypes.byref(d)) == C.OK
    assert ctypes.sizeof(C.PmDesc) == 176
    assert d.channels == 0 and d.contrast_mode == 0 and list(d.reserved) == [0, 0, 0, 0]
    # the word right after contrast_mode: the second of the four-word view
    d.channels = 3
    assert list(d.reserved) == [0, 3, 0, 0]
    d.channels, d.contrast_mode = 0, C.PM_CONTRAST_QUANTILE
    assert list(d.reserved) == [1, 0, 0, 0]
    # and in the struct's bytes: the words behind dim
    d.channels = 5
    words = np.frombuffer(bytes(d), np.int32)
    w = C.PmDesc.dim.offset // 4 + 1
    assert words.size == 44 and list(words[w:]) == [1, 5, 0, 0, 0]


def raw_create(channels):
    L = C.load()
    d = C.PmDesc()
    C.check(L.mad_pm_desc_init(ctypes.byref(d)))
    d.size[0], d.size[1], d.size[2] = 10, 9, 8
    d.channels = channels
    ctx = ctypes.c_void_p()
    rc = L.mad_pm_create(ctypes.byref(d), ctypes.byref(ctx))
    if rc != C.OK:
        raise C.MadError(rc, (L.mad_pm_last_error(None) or b"").decode())
    L.mad_pm_destroy(ctx)


@pytest.mark.parametrize("channels", [-1, 17])
def test_invalid_channel_counts(channels):
    with pytest.raises(C.MadError) as e:
        raw_create(channels)
    print(e.value)
    assert e.value.code == C.ERR_INVALID
    assert "channels" in str(e.value)


@pytest.mark.parametrize("channels", [-1, 17])
def test_python_context_refuses_invalid_channel_counts(channels):
    from multigridanisotropicdiffusion_amd import pm
    with pytest.raises(C.MadError) as e:
        pm.PM2D((9, 10), SP2, channels=channels)
    assert e.value.code == C.ERR_INVALID


class _Unbuilt:
    """A context's host-side shape checks without a device: the fields _img reads."""

    def __init__(self, cls, shape, channels):
        self.v = cls.__new__(cls)
        self.v.shape, self.v.channels = shape, channels
        self.v.image_shape = shape if channels == 1 else (channels,) + shape
        self.v._ctx = None


def test_python_contexts_reject_a_wrong_leading_axis():
    from multigridanisotropicdiffusion_amd import pm
    for cls, shape in ((pm.PM2D, (9, 10)), (pm.PM, (4, 9, 10))):
        v = _Unbuilt(cls, shape, 3).v
        assert v._img(np.zeros((3,) + shape)).shape == (3,) + shape
        for bad in (shape, (2,) + shape, shape + (3,), (3,) + shape[::-1]):
            with pytest.raises(ValueError):
                v._img(np.zeros(bad))
        with pytest.raises(ValueError):
            v.run(np.zeros((3,) + shape), channel_axis=1)
        with pytest.raises(ValueError):  # channel_axis=-1 moves the last axis first: (10, 3, 9) here
            v.run(np.zeros((3,) + shape), channel_axis=-1)
        one = _Unbuilt(cls, shape, 1).v
        with pytest.raises(ValueError):
            one._img(np.zeros((1,) + shape))
    f = pm.PeronaMalikDiffusionImageFilter()
    with pytest.raises(ValueError):
        f.SetInput(np.zeros((3, 9, 10)), channel_axis=1)
    f.SetInput(np.zeros((9, 10, 3)), channel_axis=-1)  # spacing defaulted to three axes
    with pytest.raises(ValueError):
        f.Update()


@pytest.mark.parametrize("shape,sp", [((9, 11), SP2), ((5, 6, 7), (0.8, 1.0, 1.25))])
def test_one_channel_restatement_is_the_scalar_one(shape, sp):
    img = 100.0 * synth.image(shape, seed=9)
    for kind in (P.WEICKERT, P.EXPONENTIAL, P.RATIONAL):
        D, g = P.pm_tensor(img, sp, kind, 1.0, 6.0, 2.0, 0.01)
        Dv, gv = V.pm_tensor(img[None], sp, kind, 1.0, 6.0, 2.0, 0.01)
        assert Dv.tobytes() == D.tobytes() and gv.tobytes() == g.tobytes()
    G32 = V.gradients_fp32(img[None], sp, 1.0)
    assert V.joint_s_fp32(G32).tobytes() == P.magnitude_fp32(G32[0]).tobytes()


def test_fp32_emulation_sums_the_channels_in_fp32():
    img = np.stack([100.0 * synth.image((9, 65), seed=9 + c) for c in range(3)])
    G, G32 = V.gradients(img, SP2, 1.0), V.gradients_fp32(img, SP2, 1.0)
    s, s32 = V.joint_s(G), V.joint_s_fp32(G32)
    err = np.abs(s32 - s).max() / s.max()
    print(f"joint s, fp32 emulation: {err:.3e} of max s")
    assert np.array_equal(s32, s32.astype(np.float32).astype(np.float64))
    assert 0.0 < err < 4e-6


def test_a_strong_edge_protects_a_weak_one(oracle_mod):
    """Channel 0 a noisy step of 50, channel 1 a co-located step of 4 under noise of sigma 2;
    rational diffusivity, sigma = 1.5, K = 5, alpha = 0.01, time step 2, 2 x 2 steps.  Channel by
    channel the weak step is noise to its own edge map and is blurred away; the joint diffusivity
    sees the strong channel's edge and keeps it.  Measured: weak-step jump 3.52 in the input, 1.54
    joint, 0.41 channel by channel; flat std of the weak channel 2.08 -> 0.22 (channel by channel
    0.25); monotonicity 0.53."""
    img = V.behaviour_image()
    sp = (1.0, 1.0)
    joint = V.pm_run(img, sp, oracle_mod, **V.BEHAVIOUR_KW)[-1]
    split = V.pm_run(img, sp, oracle_mod, joint=False, **V.BEHAVIOUR_KW)[-1]
    kw = V.BEHAVIOUR_KW
    mono = P.monotonicity(V.pm_tensor(img, sp, kw["diffusivity"], kw["noise_scale"], kw["contrast"], 2.0,
                                      kw["alpha"])[1])
    V.behaviour_checks(img, joint, split, mono)
