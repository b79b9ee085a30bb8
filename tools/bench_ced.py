"""Structure-tensor diffusion timing (include/mad_ced.h): the five tensor passes and the whole
filter (1 iteration, DiffusionIterations steps) on bench_ved.py's synthetic tube phantom.

    python tools/bench_ced.py [--size 256] [--steps 5] [--reps 5] [--enhancement ced] [--md FILE]

Per-pass times are HIP-event times around each kernel (mad_ced_stats.pass_ms), the best of
--reps runs by tensor time.  The roofline figure divides the pass structure's algorithmic
traffic -- 16 + 20 + 36 + 48 + 72 = 192 B per voxel in fp32 (384 in fp64 storage, less the
fp64 ends: 8 + 48 stay) -- by the tensor time, against 8 TB/s (README's convention).  Prints
one JSON line; --md also writes the table as markdown.

    python tools/bench_ced.py --dim 2 [--size 8192] ...

times the 2D path on a 2D slice of the same phantom: the fused tensor kernel (pass_ms[0]) against
its 8 + 24 = 32 algorithmic bytes per pixel (fp64 image in, fp64 tensor out, in either storage
precision) and 8 TB/s, with the diffusion time beside it.  8192^2 keeps the fp64 image at
512 MiB, beyond the 256 MiB Infinity Cache.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PASSES = ("z (sigma)", "y (sigma)", "x (sigma) + products + x (rho)", "y (rho)", "z (rho) + eigen + tensor")
HBM = 8.0e12


def pass_bytes(fp64):
    t = 8 if fp64 else 4
    return (8 + 2 * t, 2 * t + 3 * t, 3 * t + 6 * t, 6 * t + 6 * t, 6 * t + 48)


def phantom_slice(S, seed=4):
    """The plane z = S / 2 of bench_ved.phantom's construction, built without the volume: noise,
    the tubes along z as blobs, the tubes along y / x as stripes weighted by their distance from
    the plane."""
    rng = np.random.default_rng(seed)
    img = rng.normal(0.0, 10.0, size=(S, S)).astype(np.float32)
    g = np.arange(S, dtype=np.float32)
    z = np.float32(S // 2)
    for axis in range(3):
        for _ in range(64 // 3 + (1 if axis < 64 % 3 else 0)):
            a, b = rng.uniform(8, S - 8, size=2)
            r = rng.uniform(2, 6)
            if axis == 0:    # tube along z: a blob at (y, x) = (a, b), within 6 r
                y0, y1 = max(int(a - 6 * r), 0), min(int(a + 6 * r) + 2, S)
                x0, x1 = max(int(b - 6 * r), 0), min(int(b + 6 * r) + 2, S)
                img[y0:y1, x0:x1] += 200.0 * np.exp(-((g[y0:y1, None] - a) ** 2 + (g[None, x0:x1] - b) ** 2)
                                                    / (2 * r * r))
            elif axis == 1:  # along y, centred at (z, x) = (a, b): a stripe over x
                a = z + (a - z) * 16.0 / S  # keep the tube within reach of the plane
                img += 200.0 * np.exp(-((z - a) ** 2 + (g[None, :] - b) ** 2) / (2 * r * r))
            else:            # along x, centred at (z, y) = (a, b): a stripe over y
                a = z + (a - z) * 16.0 / S
                img += 200.0 * np.exp(-((z - a) ** 2 + (g[:, None] - b) ** 2) / (2 * r * r))
    return img


def main2d(a):
    import multigridanisotropicdiffusion_amd as M
    S = a.size or 8192
    img = phantom_slice(S)
    kw = dict(enhancement=a.enhancement, noise_scale=0.5, feature_scale=2.0, contrast=5.0,
              exponent=2.0, alpha=0.01, time_step=0.1)
    v = M.CED2D((S, S), (1.0, 1.0), diffusion_iterations=a.steps,
                precision=M.FP64 if a.fp64 else M.FP32, **kw)
    v.run(img, out_dtype=np.float32)  # warm-up: allocations, first launches
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        _, st = v.run(img, out_dtype=np.float32)
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        runs.append(st)
    v.close()
    best = min(runs, key=lambda r: r["tensor_ms"])
    times = sorted(r["tensor_ms"] for r in runs)
    N, B = float(S) ** 2, 32
    tw, th = best["tile"]
    R = 2 + 8  # sigma 0.5 + rho 2 at unit spacing: radii 2 + 8
    amp = (tw + 2 * R) * (th + 2 * R) / (tw * th)
    res = {
        "workload": f"{a.enhancement.upper()} {S}^2 slice of the tube phantom, sigma 0.5, rho 2, 1 iteration, "
                    f"{a.steps} diffusion steps of 0.1",
        "precision": "fp64" if a.fp64 else "fp32",
        "tensor_ms": round(best["tensor_ms"], 4),
        "tensor_ms_median": round(times[len(times) // 2], 4),
        "tile": [tw, th],
        "halo_amplification": round(amp, 3),
        "bytes_per_pixel": B,
        "tensor_TBps": round(B * N / (best["tensor_ms"] * 1e-3) / 1e12, 3),
        "fraction_of_8TBps": round(B * N / (best["tensor_ms"] * 1e-3) / HBM, 3),
        "tensor_Mpix_per_s": round(N / (best["tensor_ms"] * 1e-3) / 1e6, 1),
        "diffusion_ms": round(best["diffusion_ms"], 3),
        "cycles": best["total_cycles"], "last_relres": best["last_relres"],
        "wall_ms_incl_pcie": round(best["wall_ms"], 2),
        "tensor_ms_all_reps": [round(r["tensor_ms"], 4) for r in runs],
    }
    print(json.dumps(res), flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write(f"# Structure-tensor diffusion, 2D, {S}^2 {res['precision']}\n\n")
            f.write(f"`python tools/bench_ced.py --dim 2 --size {S} --steps {a.steps} --reps {a.reps}"
                    f"{' --fp64' if a.fp64 else ''} --enhancement {a.enhancement}` on one MI355X.\n\n")
            f.write(f"Workload: {res['workload']}.  HIP-event times after one warm-up run, best of {a.reps} runs "
                    f"by tensor time (median {res['tensor_ms_median']} ms, all runs: {res['tensor_ms_all_reps']} ms).  "
                    "Nobody had measured this kernel before: the figures record what it runs at, they are "
                    "not a target.\n\n")
            f.write("| kernel | tile | ms | B/pixel (algorithmic) | TB/s | of 8 TB/s | Mpixel/s |\n|---|---|---|---|---|---|---|\n")
            f.write(f"| ced2_k (fused tensor generation) | {tw} x {th} | {res['tensor_ms']:.4f} | {B} | "
                    f"{res['tensor_TBps']:.2f} | {res['fraction_of_8TBps']:.1%} | {res['tensor_Mpix_per_s']:.0f} |\n\n")
            f.write("The 32 B/pixel is the arithmetic of the fused kernel (8 B fp64 image in, 24 B fp64 tensor "
                    "out), not a measurement.  Each block stages its tile with the sigma + rho halo, "
                    f"({tw} + {2 * R})({th} + {2 * R}) / ({tw} x {th}) = {amp:.2f} x the 8-B input per pixel; "
                    "the re-read halo comes from L2 / Infinity Cache where a neighbouring block fetched it first.  "
                    f"The image is {N * 8 / 2**20:.0f} MiB in fp64.\n\n")
            f.write(f"Diffusion (the solver's 2D kernels, recorded, not addressed here): {res['diffusion_ms']} ms for "
                    f"{a.steps} steps (setup redone for the new tensor, {res['cycles']} cycles, last relres "
                    f"{res['last_relres']:.2e}).  Whole call with host transfers: {res['wall_ms_incl_pcie']} ms.\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3, choices=(2, 3))
    ap.add_argument("--size", type=int, default=None, help="edge length (default 256; --dim 2: 8192)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fp64", action="store_true")
    ap.add_argument("--enhancement", default="ced", choices=("eed", "ced"))
    ap.add_argument("--md", default=None, help="also write the result as a markdown file")
    a = ap.parse_args()
    if a.dim == 2:
        return main2d(a)
    import multigridanisotropicdiffusion_amd as M
    from bench_ved import phantom
    S = a.size or 256
    img = phantom(S)
    kw = dict(enhancement=a.enhancement, noise_scale=0.5, feature_scale=2.0, contrast=5.0,
              exponent=2.0, alpha=0.01, time_step=0.1)
    v = M.CED((S, S, S), (1.0, 1.0, 1.0), diffusion_iterations=a.steps,
              precision=M.FP64 if a.fp64 else M.FP32, **kw)
    v.run(img, out_dtype=np.float32)  # warm-up: allocations, first launches
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        _, st = v.run(img, out_dtype=np.float32)
        st["wall_ms"] = (time.perf_counter() - t0) * 1e3
        runs.append(st)
    v.close()
    best = min(runs, key=lambda r: r["tensor_ms"])
    N = float(S) ** 3
    pb = pass_bytes(a.fp64)
    res = {
        "workload": f"{a.enhancement.upper()} {S}^3 tube phantom, sigma 0.5, rho 2, 1 iteration, "
                    f"{a.steps} diffusion steps of 0.1",
        "precision": "fp64" if a.fp64 else "fp32",
        "tensor_ms": round(best["tensor_ms"], 4),
        "pass_ms": [round(t, 4) for t in best["pass_ms"]],
        "pass_bytes_per_voxel": list(pb),
        "bytes_per_voxel": sum(pb),
        "tensor_TBps": round(sum(pb) * N / (best["tensor_ms"] * 1e-3) / 1e12, 3),
        "fraction_of_8TBps": round(sum(pb) * N / (best["tensor_ms"] * 1e-3) / HBM, 3),
        "tensor_Mvox_per_s": round(N / (best["tensor_ms"] * 1e-3) / 1e6, 1),
        "diffusion_ms": round(best["diffusion_ms"], 3),
        "cycles": best["total_cycles"], "last_relres": best["last_relres"],
        "wall_ms_incl_pcie": round(best["wall_ms"], 2),
        "tensor_ms_all_reps": [round(r["tensor_ms"], 4) for r in runs],
    }
    print(json.dumps(res), flush=True)
    if a.md:
        with open(a.md, "w") as f:
            f.write(f"# Structure-tensor diffusion, {S}^3 {res['precision']}\n\n")
            f.write(f"`python tools/bench_ced.py --size {S} --steps {a.steps} --reps {a.reps}"
                    f"{' --fp64' if a.fp64 else ''} --enhancement {a.enhancement}` on one MI355X.\n\n")
            f.write(f"Workload: {res['workload']}.  HIP-event times, best of {a.reps} runs by tensor time "
                    f"(all runs: {res['tensor_ms_all_reps']} ms).  Nobody had measured this path before: "
                    "the figures record what it runs at, they are not a target.\n\n")
            f.write("| pass | ms | B/voxel (algorithmic) | TB/s | of 8 TB/s |\n|---|---|---|---|---|\n")
            for name, ms, b in zip(PASSES, best["pass_ms"], pb):
                bw = b * N / (ms * 1e-3)
                f.write(f"| {name} | {ms:.4f} | {b} | {bw / 1e12:.2f} | {bw / HBM:.1%} |\n")
            f.write(f"| **tensor generation** | **{res['tensor_ms']:.4f}** | **{sum(pb)}** | "
                    f"**{res['tensor_TBps']:.2f}** | **{res['fraction_of_8TBps']:.1%}** |\n\n")
            f.write(f"The {sum(pb)} B/voxel is the arithmetic of the pass structure "
                    f"({' + '.join(str(b) for b in pb)}), not a measurement; tile halos are re-read on top "
                    "of it (the last pass stages its z halo once per tile of planes).  "
                    f"One volume is {N * (8 if a.fp64 else 4) / 2**20:.0f} MiB, so part of what a pass reads "
                    "can still sit in the 256 MiB Infinity Cache from the pass that wrote it: the per-pass "
                    "rates are rates of algorithmic bytes, not HBM counters.\n\n")
            f.write(f"Diffusion: {res['diffusion_ms']} ms for {a.steps} steps (setup redone for the new tensor, "
                    f"{res['cycles']} cycles, last relres {res['last_relres']:.2e}).  "
                    f"Whole call with host transfers: {res['wall_ms_incl_pcie']} ms.\n")


if __name__ == "__main__":
    main()
