"""Perona-Malik tensor-generation timing (include/mad_pm.h) beside the structure-tensor filter's,
measured in the same run on bench_ved.py's synthetic tube phantom.

    python tools/bench_pm.py [--dim 3] [--size 256] [--reps 10] [--fp64] [--md FILE]
    python tools/bench_pm.py --dim 2 [--size 8192] ...
    python tools/bench_pm.py --quantile 0.9 [--image constant] ...
    python tools/bench_pm.py --channels 3 [--dim 2] ...   (bench_channels: joint against C scalar)

--quantile Q adds a third context in the same alternation, Perona-Malik with its contrast taken
from the Q-quantile of the gradient magnitudes (include/mad_pm.h "Contrast from a quantile"), and
reports its tensor time and the ratio to the fixed-contrast generation; --image constant times it
on a constant image (every key in one bin at every digit of the selection: the worst case).  Its
algorithmic traffic: the gradient passes with s stored instead of the tensor (T per voxel), the
selection's reads of s (two full reads, then the candidates), and the map (T in, the tensor out).

Per-pass times are HIP-event times around each kernel (mad_pm_stats.pass_ms / mad_ced_stats.pass_ms)
of whole-filter runs with one diffusion step, after one warm-up run of each filter; the two
filters alternate, and the best run by tensor time is reported with the median and every run
beside it.  The roofline figure divides the algorithmic traffic -- 3D: 16 + 20 + 60 = 96 B per
voxel in fp32 storage (EED / CED: 192); 2D: 8 + 24 = 32 B per pixel for both filters -- by the
tensor time, against 8 TB/s (README's convention).  Prints one JSON line; --md also writes the
table as markdown.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_ced  # noqa: E402  (the phantom slice and the CED pass arithmetic)

HBM = 8.0e12
PM_PASSES = ("z (sigma)", "y (sigma)", "x (sigma) + diffusivity + tensor")


def pm_pass_bytes(fp64):
    t = 8 if fp64 else 4
    return (8 + 2 * t, 2 * t + 3 * t, 3 * t + 48)


def summary(runs):
    best = min(runs, key=lambda r: r["tensor_ms"])
    times = sorted(r["tensor_ms"] for r in runs)
    return best, times[len(times) // 2], [round(r["tensor_ms"], 4) for r in runs]


def vector_bytes(dim, C, fp64):
    """(joint, C scalar generations), algorithmic bytes per voxel / pixel."""
    if dim == 2:
        return 8 * C + 24, 32 * C
    z, y, x = pm_pass_bytes(fp64)
    return (z + y) * C + (x - 48) * C + 48, (z + y + x) * C


def bench_channels(a, M, img):
    """--channels C: the joint generation of a C-channel image (include/mad_pm.h "Vector-valued
    images") against C scalar generations, and a whole run against C scalar runs, alternating in
    this process.  Channel c is the phantom rolled by 3 c along x plus 10 c, so the channels' edges
    differ.  Times are the stats' HIP-event times; a scalar figure is the sum over the channels."""
    dim, C = a.dim, a.channels
    S = img.shape[0]
    shape, sp = (S,) * dim, (1.0,) * dim
    kw = dict(noise_scale=0.5, contrast=5.0, exponent=2.0, alpha=0.01, time_step=0.1, diffusion_iterations=1,
              precision=M.FP64 if a.fp64 else M.FP32, diffusivity=a.diffusivity)
    cls = M.PM if dim == 3 else M.PM2D
    chans = np.stack([np.roll(img, 3 * c, axis=-1) + 10.0 * c for c in range(C)])
    vec, one = cls(shape, sp, channels=C, **kw), cls(shape, sp, **kw)
    vec.run(chans, out_dtype=np.float32)
    one.run(chans[0], out_dtype=np.float32)
    joint, split = [], []
    for _ in range(a.reps):
        joint.append(vec.run(chans, out_dtype=np.float32)[1])
        per = [one.run(chans[c], out_dtype=np.float32)[1] for c in range(C)]
        split.append({k: sum(p[k] for p in per) for k in ("tensor_ms", "diffusion_ms", "total_cycles")})
    vec.close()
    one.close()
    bj, bs = min(joint, key=lambda r: r["tensor_ms"]), min(split, key=lambda r: r["tensor_ms"])
    med = lambda runs, k: sorted(r[k] for r in runs)[len(runs) // 2]
    Bj, Bs = vector_bytes(dim, C, a.fp64)
    res = {"workload": f"{S}^{dim} tube phantom, {C} channels, sigma 0.5, K 5, {a.diffusivity}, 1 iteration, "
                       "1 diffusion step of 0.1", "precision": "fp64" if a.fp64 else "fp32", "channels": C,
           "joint": {"tensor_ms": round(bj["tensor_ms"], 4), "tensor_ms_median": round(med(joint, "tensor_ms"), 4),
                     "diffusion_ms": round(bj["diffusion_ms"], 3), "cycles": bj["total_cycles"], "bytes": Bj,
                     "pass_ms": [round(t, 4) for t in bj["pass_ms"]]},
           "scalar_x_C": {"tensor_ms": round(bs["tensor_ms"], 4), "tensor_ms_median": round(med(split, "tensor_ms"), 4),
                          "diffusion_ms": round(bs["diffusion_ms"], 3), "cycles": bs["total_cycles"], "bytes": Bs},
           "tensor_ratio": round(bj["tensor_ms"] / bs["tensor_ms"], 3), "tensor_ratio_predicted": round(Bj / Bs, 3),
           "run_ratio": round((med(joint, "tensor_ms") + med(joint, "diffusion_ms")) /
                              (med(split, "tensor_ms") + med(split, "diffusion_ms")), 3)}
    print(json.dumps(res), flush=True)
    if a.md:
        unit = "voxel" if dim == 3 else "pixel"
        with open(a.md, "a") as f:
            f.write(f"\n## {S}^{dim} {res['precision']}, {C} channels\n\n`python tools/bench_pm.py --dim {dim} --size {S} "
                    f"--channels {C} --reps {a.reps}{' --fp64' if a.fp64 else ''}` on one MI355X; best of {a.reps} by "
                    "tensor time (median beside it), the two alternating in one process.\n\n"
                    f"| | tensor ms (best) | median | B/{unit} (algorithmic) | diffusion ms | cycles |\n|---|---|---|---|---|---|\n")
            for label, k in (("joint generation", "joint"), (f"{C} scalar generations", "scalar_x_C")):
                r = res[k]
                f.write(f"| {label} | {r['tensor_ms']:.4f} | {r['tensor_ms_median']:.4f} | {r['bytes']} | "
                        f"{r['diffusion_ms']} | {r['cycles']} |\n")
            f.write(f"\nTensor time joint / scalar: {res['tensor_ratio']:.2f} (the byte counts alone predict "
                    f"{res['tensor_ratio_predicted']:.2f}); whole run (tensor + diffusion, medians): "
                    f"{res['run_ratio']:.2f}.\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=3, choices=(2, 3))
    ap.add_argument("--size", type=int, default=None, help="edge length (default 256; --dim 2: 8192)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fp64", action="store_true")
    ap.add_argument("--diffusivity", default="weickert", choices=("weickert", "exponential", "rational"))
    ap.add_argument("--quantile", type=float, default=None, help="also time quantile mode at this q")
    ap.add_argument("--image", default="phantom", choices=("phantom", "constant"))
    ap.add_argument("--md", default=None, help="also write the result as a markdown file")
    ap.add_argument("--channels", type=int, default=None,
                    help="time the joint generation of a C-channel image against C scalar ones (--md appends)")
    a = ap.parse_args()
    import multigridanisotropicdiffusion_amd as M
    dim = a.dim
    S = a.size or (256 if dim == 3 else 8192)
    if dim == 3:
        from bench_ved import phantom
        img = phantom(S)
    else:
        img = bench_ced.phantom_slice(S)
    if a.image == "constant":
        img = np.full_like(img, 100.0)
    if a.channels is not None:
        return bench_channels(a, M, img)
    shape, sp = (S,) * dim, (1.0,) * dim
    common = dict(noise_scale=0.5, contrast=5.0, exponent=2.0, alpha=0.01, time_step=0.1,
                  diffusion_iterations=1, precision=M.FP64 if a.fp64 else M.FP32)
    pm = (M.PM if dim == 3 else M.PM2D)(shape, sp, diffusivity=a.diffusivity, **common)
    ced = (M.CED if dim == 3 else M.CED2D)(shape, sp, enhancement="eed", feature_scale=2.0, **common)
    ctxs = [("pm", pm), ("ced", ced)]
    if a.quantile is not None:
        ctxs.append(("pm_quantile", (M.PM if dim == 3 else M.PM2D)(shape, sp, diffusivity=a.diffusivity,
                                                                   **dict(common, contrast_quantile=a.quantile))))
    for _, v in ctxs:  # warm-up: allocations, first launches
        v.run(img, out_dtype=np.float32)
    runs = {name: [] for name, _ in ctxs}
    for _ in range(a.reps):
        for name, v in ctxs:
            runs[name].append(v.run(img, out_dtype=np.float32)[1])
    for _, v in ctxs:
        v.close()
    N = float(S) ** dim
    unit = "voxel" if dim == 3 else "pixel"
    bytes_pm = sum(pm_pass_bytes(a.fp64)) if dim == 3 else 32
    bytes_ced = sum(bench_ced.pass_bytes(a.fp64)) if dim == 3 else 32
    res = {"workload": f"{S}^{dim} tube phantom, sigma 0.5, K 5, {a.diffusivity} (EED beside it: rho 2), "
                       "1 iteration, 1 diffusion step of 0.1",
           "precision": "fp64" if a.fp64 else "fp32"}
    rows = []
    for name, B in (("pm", bytes_pm), ("ced", bytes_ced)):
        best, med, allr = summary(runs[name])
        bw = B * N / (best["tensor_ms"] * 1e-3)
        res[name] = {"tensor_ms": round(best["tensor_ms"], 4), "tensor_ms_median": round(med, 4),
                     "pass_ms": [round(t, 4) for t in best["pass_ms"]], "tile": list(best["tile"]),
                     f"bytes_per_{unit}": B, "tensor_TBps": round(bw / 1e12, 3),
                     "fraction_of_8TBps": round(bw / HBM, 3),
                     f"tensor_M{unit[:3]}_per_s": round(N / (best["tensor_ms"] * 1e-3) / 1e6, 1),
                     "diffusion_ms": round(best["diffusion_ms"], 3), "cycles": best["total_cycles"],
                     "tensor_ms_all_reps": allr}
        rows.append((name, best, B, bw))
    res["pm_over_ced"] = round(res["pm"]["tensor_ms"] / res["ced"]["tensor_ms"], 3)
    if a.quantile is not None:
        # s stored and re-read by the map, two full reads by the selection (the candidates on top)
        t = 8 if a.fp64 else 4
        Bq = bytes_pm + 4 * t
        best, med, allr = summary(runs["pm_quantile"])
        bw = Bq * N / (best["tensor_ms"] * 1e-3)
        res["image"] = a.image
        res["pm_quantile"] = {"q": a.quantile, "contrast_used": best["contrast_used"],
                              "tensor_ms": round(best["tensor_ms"], 4), "tensor_ms_median": round(med, 4),
                              "pass_ms": [round(x, 4) for x in best["pass_ms"]],
                              f"bytes_per_{unit}": Bq, "tensor_TBps": round(bw / 1e12, 3),
                              "tensor_ms_all_reps": allr}
        res["quantile_over_fixed"] = round(best["tensor_ms"] / res["pm"]["tensor_ms"], 3)
        res["quantile_over_fixed_median"] = round(med / res["pm"]["tensor_ms_median"], 3)
    print(json.dumps(res), flush=True)
    if not a.md:
        return
    with open(a.md, "w") as f:
        f.write(f"# Perona-Malik tensor generation, {S}^{dim} {res['precision']}\n\n")
        f.write(f"`python tools/bench_pm.py --dim {dim} --size {S} --reps {a.reps}{' --fp64' if a.fp64 else ''} "
                f"--diffusivity {a.diffusivity}` on one MI355X.\n\n")
        f.write(f"Workload: {res['workload']}.  HIP-event times of whole-filter runs after one warm-up run of each "
                f"filter, the two filters alternating; best of {a.reps} runs by tensor time.  Nobody had measured "
                "these kernels before: the figures record what they run at, they are not a target.\n\n")
        f.write(f"| filter | tile | tensor ms (best) | median | B/{unit} (algorithmic) | TB/s | of 8 TB/s | M{unit}/s |\n"
                "|---|---|---|---|---|---|---|---|\n")
        for name, best, B, bw in rows:
            label = "Perona-Malik" if name == "pm" else "EED (same run)"
            tile = "{} x {}".format(*best["tile"]) if dim == 2 else "-"
            f.write(f"| {label} | {tile} | {best['tensor_ms']:.4f} | {res[name]['tensor_ms_median']:.4f} | {B} | "
                    f"{bw / 1e12:.2f} | {bw / HBM:.1%} | {N / (best['tensor_ms'] * 1e-3) / 1e6:.0f} |\n")
        f.write(f"\nPerona-Malik takes {res['pm_over_ced']:.2f} x the EED generation's time.  All runs, ms: "
                f"Perona-Malik {res['pm']['tensor_ms_all_reps']}, EED {res['ced']['tensor_ms_all_reps']}.\n\n")
        if a.quantile is not None:
            q = res["pm_quantile"]
            f.write(f"Contrast from the {a.quantile} quantile ({a.image} image): {q['tensor_ms']:.4f} ms (median "
                    f"{q['tensor_ms_median']:.4f}), {res['quantile_over_fixed']:.2f} x the fixed-contrast generation, "
                    f"K = {q['contrast_used']:.6g}; pass_ms {q['pass_ms']} (the selection and the map count with the "
                    f"last pass); all runs, ms: {q['tensor_ms_all_reps']}.\n\n")
        if dim == 3:
            f.write("| Perona-Malik pass | ms | B/voxel (algorithmic) | TB/s | of 8 TB/s |\n|---|---|---|---|---|\n")
            for pname, ms, b in zip(PM_PASSES, rows[0][1]["pass_ms"], pm_pass_bytes(a.fp64)):
                bw = b * N / (ms * 1e-3)
                f.write(f"| {pname} | {ms:.4f} | {b} | {bw / 1e12:.2f} | {bw / HBM:.1%} |\n")
            f.write("\n| EED pass | ms | B/voxel (algorithmic) | TB/s | of 8 TB/s |\n|---|---|---|---|---|\n")
            for pname, ms, b in zip(bench_ced.PASSES, rows[1][1]["pass_ms"], bench_ced.pass_bytes(a.fp64)):
                bw = b * N / (ms * 1e-3)
                f.write(f"| {pname} | {ms:.4f} | {b} | {bw / 1e12:.2f} | {bw / HBM:.1%} |\n")
            f.write("\nThe bytes per voxel are the arithmetic of the pass structures, not a measurement; tile halos "
                    f"are re-read on top of them.  One volume is {N * (8 if a.fp64 else 4) / 2**20:.0f} MiB, so part "
                    "of what a pass reads can still sit in the 256 MiB Infinity Cache from the pass that wrote it: "
                    "the per-pass rates are rates of algorithmic bytes, not HBM counters.  The z and y passes are "
                    "the same kernels in both filters.\n\n")
        else:
            f.write("The 32 B/pixel is the arithmetic of either fused kernel (8 B fp64 image in, 24 B fp64 tensor "
                    f"out), not a measurement; each block re-reads its halo on top of it.  The image is "
                    f"{N * 8 / 2**20:.0f} MiB in fp64.\n\n")
        f.write(f"Diffusion (one step, setup redone for the new tensor; recorded, not addressed here): Perona-Malik "
                f"{res['pm']['diffusion_ms']} ms (cycles: {res['pm']['cycles']}, the isotropic operator), EED "
                f"{res['ced']['diffusion_ms']} ms (cycles: {res['ced']['cycles']}, the full operator).\n")


if __name__ == "__main__":
    main()
