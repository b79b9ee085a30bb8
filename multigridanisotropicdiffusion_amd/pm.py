"""Regularised Perona-Malik (nonlinear isotropic) diffusion on the GPU, a sibling of the
structure-tensor filters (ced.py).

The diffusion tensor is g I with a scalar diffusivity g of the squared gradient at the noise
scale (Catte's regularisation); the implicit MAD steps are stable at time steps of 1-10, where
the explicit ITK anisotropic-diffusion filters are capped near 0.06-0.125 (definition:
include/mad_pm.h).  Everything -- the tensor passes and the MAD diffusion steps -- runs in
libmad_hip.so; there is no CPU fallback.

The solver's stencil keeps the maximum principle where the diffusivity varies gently,
|g(p + 1) - g(p - 1)| <= 4 g(p); a noise scale of 1-2 grid spacings, the rational diffusivity
or a larger alpha keep it (include/mad_pm.h, "Monotonicity").

``PM`` is the low-level context (one image size) for volumes, ``PM2D`` the same for 2D images
(one fused tensor kernel); ``PeronaMalikDiffusionImageFilter`` the ITK-shaped facade.  All three
take vector-valued images (``channels=C``, ``SetInput(image, channel_axis=...)``): colour pictures
and multi-echo volumes with one joint diffusivity from the summed squared gradients of all
channels, so an edge that one channel shows clearly is kept in every channel.
"""
import ctypes

import numpy as np

from . import _capi as C
from .filters import Image, MultigridGaussSeidelSmoother
from .solver import mad_dtype

_DIFF = {"weickert": C.PM_WEICKERT, "exponential": C.PM_EXPONENTIAL, "rational": C.PM_RATIONAL}


def _diffusivity(v):
    if isinstance(v, str):
        try:
            return _DIFF[v.lower()]
        except KeyError:
            raise ValueError(f"diffusivity {v!r}: 'weickert', 'exponential' or 'rational'") from None
    return int(v)


class _Context:
    """One mad_pm_ctx of dimension DIM (the body PM and PM2D share).  shape: numpy, x last;
    spacing x first.  diffusivity: "weickert" / "exponential" / "rational" (or C.PM_*).
    contrast_quantile=q (0 < q <= 1) overrides contrast: every tensor generation takes K^2 as the
    q-quantile of the squared gradient magnitudes, selected on the device (include/mad_pm.h,
    "Contrast from a quantile"); run then reports the last K as stats["contrast_used"].  The
    attribute contrast_used holds the K of the last run in both modes: run sets it, it is None
    before the first run, and 0.0 after a quantile-mode run with iterations = 0 (no generation).
    _contrast_squared is for tests only: an absolute K^2 fed to the map unsquared
    (MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED).
    channels=C > 1: vector-valued images with one joint diffusivity (include/mad_pm.h,
    "Vector-valued images").  Images are (C,) + shape, or with run's channel_axis=-1 shape + (C,);
    tensor() returns the joint tensor, gradient() (C, dim) + shape, and run's stats dict adds
    "channels"."""

    DIM = None

    def __init__(self, shape, spacing=None, *, diffusivity="weickert", noise_scale=0.5, contrast=1.0,
                 exponent=2.0, alpha=0.01, iterations=1, diffusion_iterations=5, cycle=C.VCYCLE,
                 time_step=0.1, tolerance=1e-6, diffusion_iterations_per_grid=2, verbose=False,
                 smoother=C.GAUSS_SEIDEL, precision=C.PRECISION_AUTO, device=-1, contrast_quantile=None,
                 channels=1, _contrast_squared=None):
        dim = self.DIM
        if len(shape) != dim:
            raise ValueError(f"{type(self).__name__} takes a {dim}D shape (PM: volumes, PM2D: images)")
        self._L = C.load()
        self.shape = tuple(int(v) for v in shape)
        self.channels = int(channels)
        # the shape of an image argument: one channel keeps the plain shape
        self.image_shape = self.shape if self.channels == 1 else (self.channels,) + self.shape
        self.ncomp = dim * (dim + 1) // 2
        d = C.PmDesc()
        C.check(self._L.mad_pm_desc_init(ctypes.byref(d)))
        d.dim = dim
        for q, n in enumerate(reversed(self.shape)):
            d.size[q] = n
        for q in range(dim):
            d.spacing[q] = float(spacing[q]) if spacing is not None else 1.0
        d.diffusivity = _diffusivity(diffusivity)
        d.noise_scale = float(noise_scale)
        d.contrast, d.exponent, d.alpha = float(contrast), float(exponent), float(alpha)
        d.iterations, d.diffusion_iterations = int(iterations), int(diffusion_iterations)
        d.cycle, d.time_step, d.tolerance = int(cycle), float(time_step), float(tolerance)
        d.diffusion_iterations_per_grid = int(diffusion_iterations_per_grid)
        d.verbose = int(bool(verbose))
        d.smoother, d.precision, d.device = int(smoother), int(precision), int(device)
        if contrast_quantile is not None and _contrast_squared is not None:
            raise ValueError("contrast_quantile and _contrast_squared exclude each other")
        if contrast_quantile is not None:
            d.contrast_mode, d.contrast = C.PM_CONTRAST_QUANTILE, float(contrast_quantile)
        elif _contrast_squared is not None:
            d.options, d.contrast = C.PM_OPT_TEST_CONTRAST_IS_SQUARED, float(_contrast_squared)
        d.channels = self.channels
        self.quantile = contrast_quantile is not None
        # K of the last run's last tensor generation: set by run() only (None before the first run;
        # tensor() does not set it -- contrast(image, q) gives the K a quantile-mode tensor() takes)
        self.contrast_used = None
        self.desc = d
        ctx = ctypes.c_void_p()
        rc = self._L.mad_pm_create(ctypes.byref(d), ctypes.byref(ctx))
        if rc != C.OK:
            raise C.MadError(rc, (self._L.mad_pm_last_error(None) or b"").decode())
        self._ctx = ctx

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.mad_pm_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        self.close()

    def _check(self, rc):
        if rc != C.OK:
            raise C.MadError(rc, (self._L.mad_pm_last_error(self._ctx) or b"").decode())

    def _img(self, image):
        img = np.ascontiguousarray(image)
        if img.shape != self.image_shape:
            raise ValueError(f"image shape {img.shape} != {self.image_shape}")
        return img

    def run(self, image, out_dtype=np.float64, channel_axis=0):
        """The whole filter on a host image; returns (output, stats dict).  channels > 1:
        channel_axis=0 takes (C,) + shape, channel_axis=-1 pictures of shape + (C,) (made planar
        on the host); the output comes back in the layout it was given."""
        if channel_axis not in (0, -1):
            raise ValueError("channel_axis: 0 or -1")
        last = self.channels > 1 and channel_axis == -1
        img = self._img(np.moveaxis(np.asarray(image), -1, 0) if last else image)
        out = np.empty(self.image_shape, dtype=out_dtype)
        st = C.PmStats()
        rc = C.check(self._L.mad_pm_run(self._ctx, img.ctypes.data_as(ctypes.c_void_p),
                                        mad_dtype(img.dtype), out.ctypes.data_as(ctypes.c_void_p),
                                        mad_dtype(out_dtype), ctypes.byref(st)),
                     self._ctx, warn_not_converged=True, last_error=self._L.mad_pm_last_error)
        stats = st.as_dict()
        stats["converged"] = rc == C.OK
        # K of the last tensor generation.  The attribute holds it in both modes; the dict names
        # it where it is a result (quantile mode) and keeps its keys in absolute mode.
        self.contrast_used = st.contrast_used
        if self.quantile:
            stats["contrast_used"] = st.contrast_used
        if self.channels > 1:
            stats["channels"] = self.channels
        if last:
            out = np.ascontiguousarray(np.moveaxis(out, 0, -1))
        return out, stats

    def tensor(self, image, with_diffusivity=False):
        """One tensor generation: SoA tensor (6, z, y, x) [xx,xy,xz,yy,yz,zz] or (3, y, x)
        [xx,xy,yy]; with_diffusivity: (tensor, g of the image's shape)."""
        img = self._img(image)
        T = np.empty((self.ncomp,) + self.shape)
        g = np.empty(self.shape) if with_diffusivity else None
        dp = ctypes.POINTER(ctypes.c_double)
        self._check(self._L.mad_pm_tensor(self._ctx, img.ctypes.data_as(ctypes.c_void_p),
                                          mad_dtype(img.dtype), T.ctypes.data_as(dp),
                                          g.ctypes.data_as(dp) if with_diffusivity else None))
        return (T, g) if with_diffusivity else T

    def gradient(self, image):
        """The gradient at the noise scale: (3, z, y, x) (gx, gy, gz) or (2, y, x) (gx, gy);
        channels > 1: (C, dim) + shape."""
        img = self._img(image)
        G = np.empty((() if self.channels == 1 else (self.channels,)) + (self.DIM,) + self.shape)
        self._check(self._L.mad_pm_gradient(
            self._ctx, img.ctypes.data_as(ctypes.c_void_p), mad_dtype(img.dtype),
            G.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        return G


    def contrast(self, image, q):
        """K = sqrt(s_q) a quantile-mode tensor generation of this image takes for the quantile q
        (mad_pm_contrast; either contrast mode)."""
        img = self._img(image)
        K = ctypes.c_double()
        self._check(self._L.mad_pm_contrast(self._ctx, img.ctypes.data_as(ctypes.c_void_p),
                                            mad_dtype(img.dtype), float(q), ctypes.byref(K)))
        return K.value

    def select(self, values, k):
        """The k-th smallest (0-based) of the non-negative finite values, selected on the device
        (mad_pm_select): the same bits as np.partition(values, k)[k]."""
        a = np.ascontiguousarray(values, dtype=np.float64).ravel()
        out = ctypes.c_double()
        self._check(self._L.mad_pm_select(self._ctx, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                          a.size, int(k), ctypes.byref(out)))
        return out.value


class PM(_Context):
    """The 3D context.  shape: numpy (z, y, x); spacing (hx, hy, hz)."""
    DIM = 3


class PM2D(_Context):
    """The 2D context (mad_pm_desc.dim = 2).  shape: numpy (y, x); spacing (hx, hy); tensor
    (3, y, x) [xx,xy,yy]."""
    DIM = 2


class PeronaMalikDiffusionImageFilter:
    """ITK-shaped facade of regularised Perona-Malik diffusion (defaults of mad_pm_desc_init).
    SetConductanceParameter / SetNumberOfIterations, the names of ITK's anisotropic-diffusion
    family, are aliases of SetContrast / SetIterations."""

    WEICKERT, EXPONENTIAL, RATIONAL = C.PM_WEICKERT, C.PM_EXPONENTIAL, C.PM_RATIONAL
    VCYCLE, FMG, SMOOTHER = C.VCYCLE, C.FMG, C.SMOOTHER

    def __init__(self, smoother=MultigridGaussSeidelSmoother, output_dtype=None,
                 precision=C.PRECISION_AUTO, device=-1):
        self._smoother = smoother
        self._output_dtype = output_dtype
        self._precision = precision
        self._device = device
        self._p = dict(diffusivity=C.PM_WEICKERT, noise_scale=0.5, contrast=1.0, exponent=2.0,
                       alpha=0.01, iterations=1, diffusion_iterations=5, cycle=C.VCYCLE,
                       time_step=0.1, tolerance=1e-6, diffusion_iterations_per_grid=2, verbose=False,
                       contrast_quantile=None)
        self._contrast_used = None
        self._input = None
        self._channel_axis = None
        self._output = None
        self.stats = None

    @classmethod
    def New(cls, **kw):
        return cls(**kw)

    def SetDiffusivity(self, v): self._p["diffusivity"] = _diffusivity(v)
    def SetNoiseScale(self, v): self._p["noise_scale"] = float(v)
    def SetContrast(self, v):
        """An absolute contrast K (leaves quantile mode)."""
        self._p["contrast"] = float(v)
        self._p["contrast_quantile"] = None

    def SetContrastQuantile(self, q):
        """K from the q-quantile of the gradient magnitudes, per iteration (0 < q <= 1; Perona and
        Malik: 0.9)."""
        self._p["contrast_quantile"] = float(q)

    def GetContrastUsed(self):
        """K of the last tensor generation of the last Update (None before it)."""
        return self._contrast_used

    def SetExponent(self, v): self._p["exponent"] = float(v)
    def SetAlpha(self, v): self._p["alpha"] = float(v)
    def SetIterations(self, v): self._p["iterations"] = int(v)
    def SetDiffusionIterations(self, v): self._p["diffusion_iterations"] = int(v)
    def SetTimeStep(self, v): self._p["time_step"] = float(v)
    def SetTolerance(self, v): self._p["tolerance"] = float(v)
    def SetCycle(self, v): self._p["cycle"] = int(v)
    def SetDiffusionIterationsPerGrid(self, v): self._p["diffusion_iterations_per_grid"] = int(v)
    def SetVerbose(self, v): self._p["verbose"] = bool(v)
    SetConductanceParameter = SetContrast
    SetNumberOfIterations = SetIterations

    def SetInput(self, image, channel_axis=None):
        """channel_axis (0 or -1): a vector-valued image; its array carries one axis more than
        its spacing, the channels, and the output keeps that layout."""
        if channel_axis not in (None, 0, -1):
            raise ValueError("channel_axis: None, 0 or -1")
        self._input = image if isinstance(image, Image) else Image(image)
        self._channel_axis = channel_axis

    def GetOutput(self):
        return self._output

    def Update(self):
        """Run the filter on the GPU; the output pixel type is the input's unless
        output_dtype was given; spacing and origin carry over.  The input's dimension picks
        the 2D or the 3D context."""
        if self._input is None:
            raise RuntimeError("SetInput must be called before Update")
        img = self._input
        out_dtype = self._output_dtype or img.array.dtype
        ax = self._channel_axis
        if ax is None:
            shape, channels, dim = img.array.shape, 1, img.dim
        else:
            shape = img.array.shape[1:] if ax == 0 else img.array.shape[:-1]
            channels, dim = img.array.shape[ax], img.array.ndim - 1
            if len(img.spacing) != dim:
                raise ValueError("with channel_axis the array carries one axis more than the spacing")
        ctx = PM2D if dim == 2 else PM
        v = ctx(shape, img.spacing, smoother=self._smoother.smoother_id,
                precision=self._precision, device=self._device, channels=channels, **self._p)
        try:
            out, stats = v.run(img.array, out_dtype=out_dtype, channel_axis=ax or 0)
        finally:
            v.close()
        self.stats = stats
        self._contrast_used = v.contrast_used
        self._output = Image(out, spacing=img.spacing, origin=img.origin)
        return self._output
