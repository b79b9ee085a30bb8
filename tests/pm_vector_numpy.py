"""Vector-valued Perona-Malik diffusion (include/mad_pm.h, "Vector-valued images"), fp64 numpy
restatement -- TEST INFRASTRUCTURE ONLY.  The package never imports this module.

Built on tests/pm_numpy.py.  Images are (C,) + shape, channel first:

  1. gradient at the noise scale per channel (pm_numpy.gradient)
  2. s_c per channel (pm_numpy.magnitude), then s = s_0 + s_1 + ... + s_{C-1}, left to right
  3.-4. pm_numpy's map on the joint s: one g, one D = g I for all channels
  5. per outer iteration one joint tensor, then every channel through the C MAD oracle's implicit
     steps on that tensor

joint_s_fp32 is the fp32 emulation: pm_numpy.gradient_fp32 per channel, s_c and the channel sum
in fp32, left to right.
"""
import numpy as np

import pm_numpy as P


def gradients(img, spacing, sigma):
    """(C, dim) + shape."""
    return np.stack([np.stack(P.gradient(u, spacing, sigma)) for u in img])


def gradients_fp32(img, spacing, sigma):
    return np.stack([np.stack(P.gradient_fp32(u, spacing, sigma)) for u in img])


def joint_s(G):
    """s of per-channel gradients (C, dim) + shape, fp64, summed left to right."""
    s = P.magnitude(G[0])
    for g in G[1:]:
        s = s + P.magnitude(g)
    return s


def joint_s_fp32(G32):
    """The same of fp32 gradients (fp64 arrays holding fp32 values), every sum in fp32."""
    s = P.magnitude_fp32(G32[0]).astype(np.float32)
    for g in G32[1:]:
        s = s + P.magnitude_fp32(g).astype(np.float32)
    assert s.dtype == np.float32
    return s.astype(np.float64)


def pm_tensor(img, spacing, diffusivity_kind=P.WEICKERT, noise_scale=0.5, contrast=1.0, exponent=2.0,
              alpha=0.01):
    """(D, g) of the joint diffusivity; img is (C,) + shape."""
    img = np.asarray(img, np.float64)
    g = P.diffusivity(joint_s(gradients(img, spacing, noise_scale)), diffusivity_kind, contrast, exponent,
                      alpha)
    return P.tensor_from_diffusivity(g), g


def oracle_steps(oracle_mod, x, T, spacing, p):
    """Every channel of x through the oracle's implicit steps on the one tensor T:
    (iterate, cycles summed over the channels)."""
    out, cycles = np.empty_like(x), 0
    for c in range(x.shape[0]):
        o = oracle_mod.Oracle(x.shape[1:], spacing, T, p["time_step"])
        out[c], cyc, _ = o.run(x[c], cycle=p.get("cycle", oracle_mod.VCYCLE),
                               smoother=p.get("smoother", oracle_mod.GS_LEX),
                               iterations_per_grid=p["diffusion_iterations_per_grid"], max_cycles=100,
                               number_of_steps=p["diffusion_iterations"], tolerance=p["tolerance"])
        cycles += int(np.sum(cyc))
    return out, cycles


def pm_run(img, spacing, oracle_mod, joint=True, **kw):
    """The outer loop: the list of iterates, one per outer iteration.  joint=False runs the scalar
    filter channel by channel, each channel with its own tensor (what the joint diffusivity is
    compared against)."""
    p = dict(P.DEFAULTS)
    p.update(kw)
    x = np.asarray(img, np.float64).copy()
    iterates = []
    for _ in range(p["iterations"]):
        args = (spacing, p["diffusivity"], p["noise_scale"], p["contrast"], p["exponent"], p["alpha"])
        if joint:
            x, _ = oracle_steps(oracle_mod, x, pm_tensor(x, *args)[0], spacing, p)
        else:
            x = np.stack([oracle_steps(oracle_mod, x[c:c + 1], P.pm_tensor(x[c], *args)[0], spacing, p)[0][0]
                          for c in range(x.shape[0])])
        iterates.append(x.copy())
    return iterates


# ---------------------------------------------------------------- the behaviour case

BEHAVIOUR_SHAPE = (20, 24)
BEHAVIOUR_KW = dict(diffusivity=P.RATIONAL, noise_scale=1.5, contrast=5.0, alpha=0.01, time_step=2.0,
                    iterations=2, diffusion_iterations=2)


def behaviour_image():
    """Channel 0: the behaviour tests' noisy step of 50 (tests/test_gpu_pm2d.py); channel 1: a
    co-located weak step of 4 plus noise of standard deviation 2."""
    shape = BEHAVIOUR_SHAPE
    x = np.arange(shape[1])
    strong = np.where(x >= 12, 150.0, 100.0) + np.random.default_rng(3).normal(0.0, 2.0, size=shape)
    weak = np.where(x >= 12, 4.0, 0.0) + np.random.default_rng(4).normal(0.0, 2.0, size=shape)
    return np.stack([strong, weak])


def jump(u):
    """The mean jump across the edge."""
    return float((u[:, 12] - u[:, 11]).mean())


def flat(u):
    """The larger standard deviation of the two flat regions."""
    return float(max(u[:, :8].std(), u[:, 16:].std()))


def behaviour_checks(img, joint, split, mono):
    """The assertions of the behaviour case, each figure printed first: joint / split are the
    outputs of the joint diffusivity and of the scalar filter channel by channel, mono
    pm_numpy.monotonicity of the first joint diffusivity.  tests/test_pm_vector_cpu.py runs them
    on the restatement + oracle, tests/test_gpu_pm_vector.py on the GPU."""
    weak_in, weak_joint, weak_split = jump(img[1]), jump(joint[1]), jump(split[1])
    print(f"weak-step jump: input {weak_in:.2f}, joint {weak_joint:.2f}, channel by channel {weak_split:.2f}")
    print(f"strong-step jump: input {jump(img[0]):.2f}, joint {jump(joint[0]):.2f}, "
          f"channel by channel {jump(split[0]):.2f}")
    print(f"flat std of the weak channel: input {flat(img[1]):.3f}, joint {flat(joint[1]):.3f}, "
          f"channel by channel {flat(split[1]):.3f}")
    print(f"monotonicity of the first joint tensor: {mono:.3f}")
    assert weak_joint >= 2.0 * weak_split, (weak_joint, weak_split)
    assert flat(joint[1]) < flat(img[1])
    for c in range(2):
        print(f"channel {c}: input [{img[c].min():.2f}, {img[c].max():.2f}], "
              f"joint [{joint[c].min():.2f}, {joint[c].max():.2f}]")
        assert img[c].min() <= joint[c].min() and joint[c].max() <= img[c].max(), c
    assert mono <= 1.0, mono
