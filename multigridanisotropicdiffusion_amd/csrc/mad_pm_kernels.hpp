// mad_pm_kernels.hpp -- device kernels of the regularised Perona-Malik tensor
// (include/mad_pm.h): the gradient at the noise scale, its squared magnitude and a pointwise
// diffusivity, D = g I.
//
// 3D: the gradient passes of the structure-tensor filter plus one new pass.  Storage and FIR
// arithmetic in T (fp32, or fp64 in MAD_FP64) with explicit fma and contraction off; the
// diffusivity and the tensor are fp64 in every mode.
//   1. ced_z_k    image (fp64)        -> K0z u, K1z u                               8 + 2 T
//   2. ced_y_k    those two           -> K0y K0z u, K1y K0z u, K0y K1z u            2 T + 3 T
//   3. pm_x_k     those three         -> gradient (LDS and registers only), s, g,   3 T + 48
//                 the six tensor components
// Algorithmic traffic in fp32: 16 + 20 + 60 = 96 B per voxel (EED / CED: 192).
// 2D images take one fused kernel, pm2_k at the end of this file: 8 + 24 = 32 B per pixel.
// Quantile mode (contrast from a gradient quantile) splits the last step: pm_x_k / pm2_k in the
// mode PM_SQNORM store s alone (T per voxel), mad_select.hpp selects s_q, and pm_map_k maps
// s -> g -> D with K^2 = s_q read from device memory.
// Vector-valued images (C > 1 channels, one joint diffusivity) take pmv_x_k / pm2v_k at the end of
// this file in place of pm_x_k / pm2_k: 48 C + 48 B per voxel (fp32), 8 C + 24 B per pixel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mad_ced_kernels.hpp"

namespace mad {

struct PmParams {
  int diffusivity;  // MAD_PM_WEICKERT / MAD_PM_EXPONENTIAL / MAD_PM_RATIONAL
  double k2;        // contrast^2
  double m;         // exponent (Weickert only)
  double alpha;
};

enum { PM_TENSOR = 0, PM_GRADIENT = 1, PM_SQNORM = 2 };

// g(s) = alpha + (1 - alpha) g0(s), fp64; the default exponent 2 (and 1) skips pow, as ced2_stop
__device__ inline double pm_diffusivity(double s, const PmParams& pp) {
#pragma clang fp contract(off)
  double g0;
  if (pp.diffusivity == 0) {
    if (s > 0.0) {
      const double x = pp.k2 / s;
      g0 = 1.0 - exp(-(pp.m == 2.0 ? x * x : pp.m == 1.0 ? x : pow(x, pp.m)));
    } else {
      g0 = 1.0;
    }
  } else if (pp.diffusivity == 1) {
    g0 = exp(-(s / pp.k2));
  } else {
    g0 = 1.0 / (1.0 + s / pp.k2);
  }
  return pp.alpha + (1.0 - pp.alpha) * g0;
}

// Quantile mode's map: K^2 = s_q comes from the selection.  s_q = 0 (a constant image, or more
// than the share q of the voxels flat) takes the limit K -> 0+ of all three functions, g0 = 1
// where s = 0 and 0 elsewhere, instead of their 0 / 0; otherwise the function above.
__device__ inline double pm_diffusivity_selected(double s, const PmParams& pp) {
#pragma clang fp contract(off)
  if (pp.k2 == 0.0) return pp.alpha + (1.0 - pp.alpha) * (s == 0.0 ? 1.0 : 0.0);
  return pm_diffusivity(s, pp);
}

// Pointwise map of quantile mode, s -> g -> D: s (storage precision, from a PM_SQNORM pass) and
// K^2 from device memory (the selection's result; pp.k2 is ignored) to the SoA tensor with
// component stride cs (ncomp 6: [xx,xy,xz,yy,yz,zz], 3: [xx,xy,yy]) and, optionally, g.
// T in, 8 ncomp out: 52 B per voxel in 3D fp32, 28 B per pixel in 2D fp32.
template <typename T, int NCOMP>
__global__ void __launch_bounds__(256) pm_map_k(const T* __restrict__ s, const double* __restrict__ k2,
                                                int64_t n, int64_t cs, double* __restrict__ D,
                                                double* __restrict__ gout, PmParams pp) {
  pp.k2 = *k2;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    const double g = pm_diffusivity_selected((double)s[p], pp);
    D[p] = g;
    D[cs + p] = 0.0;
    if (NCOMP == 6) {
      D[2 * cs + p] = 0.0;
      D[3 * cs + p] = g;
      D[4 * cs + p] = 0.0;
      D[5 * cs + p] = g;
    } else {
      D[2 * cs + p] = g;
    }
    if (gout) gout[p] = g;
  }
}

// x pass fused with the magnitude, the diffusivity and the tensor.  Block = 256 consecutive x
// of one row.  LDS: the three input rows over [x0 - R, x0 + 256 + R), taken at the CLAMPED
// positions, so a voxel's taps read [i - R, i + R] of the replicated row for any nx (the last
// block may be narrower than R).  taps = [K0 | K1] of sigma (2 R + 1 each).
// ih = (1 / hx, 1 / hy, 1 / hz), each applied once to its gradient component.
// PM_TENSOR: D = the six tensor components (stride cs), gout (optional) = g.
// PM_GRADIENT: D = gx, gy, gz (stride cs).
// PM_SQNORM: D is read as T*: s in the storage precision and nothing else (quantile mode).
template <typename T, int MODE>
__global__ void __launch_bounds__(256) pm_x_k(const T* __restrict__ a00, const T* __restrict__ a10,
                                              const T* __restrict__ a01, const T* __restrict__ taps,
                                              int R, int nx, int ny, int nz, T ihx, T ihy, T ihz,
                                              int64_t cs, double* __restrict__ D,
                                              double* __restrict__ gout, PmParams pp) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* L = reinterpret_cast<T*>(ved_smem);
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * 256;
  const int i = x0 + tid;
  const int64_t row = ((int64_t)blockIdx.z * ny + blockIdx.y) * nx;
  const int nw = 256 + 2 * R;
  for (int e = tid; e < nw; e += 256) {
    const int64_t q = row + min(max(x0 - R + e, 0), nx - 1);
    L[e] = a00[q];
    L[nw + e] = a10[q];
    L[2 * nw + e] = a01[q];
  }
  __syncthreads();
  if (i >= nx) return;
  const int W = 2 * R + 1;
  const T* c = L + tid;
  T gx = T(0), gy = T(0), gz = T(0);
#pragma unroll 4
  for (int q = 0; q < W; ++q) {
    const T k0 = taps[q], k1 = taps[W + q];
    gx = fma(k1, c[q], gx);
    gy = fma(k0, c[nw + q], gy);
    gz = fma(k0, c[2 * nw + q], gz);
  }
  gx = gx * ihx;
  gy = gy * ihy;
  gz = gz * ihz;
  const int64_t p = row + i;
  if (MODE == PM_GRADIENT) {
    D[p] = (double)gx;
    D[cs + p] = (double)gy;
    D[2 * cs + p] = (double)gz;
    return;
  }
  T s = gx * gx;
  s = s + gy * gy;
  s = s + gz * gz;
  if (MODE == PM_SQNORM) {
    reinterpret_cast<T*>(D)[p] = s;
    return;
  }
  const double g = pm_diffusivity((double)s, pp);
  D[p] = g;
  D[cs + p] = 0.0;
  D[2 * cs + p] = 0.0;
  D[3 * cs + p] = g;
  D[4 * cs + p] = 0.0;
  D[5 * cs + p] = g;
  if (gout) gout[p] = g;
}

// ---------------------------------------------------------------------------------------
// 2D: one fused kernel per tensor generation, modelled on phases A-C of ced2_k.  The halo is
// the sigma radius alone, so the full 64 x 32 tile stays under half a CU's LDS.
//
// Block = 256 threads, a TW x TH output tile at (x0, y0); TW a power of two >= 4, TH a multiple
// of 4.  LDS holds two regions that the phases use in turn (S1 = the size of the first in
// elements, from the host):
//   A  R1  image tile WA x HA = (TW + 2 Rx) x (TH + 2 Ry), clamped, fp64 -> T
//   B  R2  K0y u, K1y u on the tile's TH rows, all WA staged columns, stored column-major with
//          the odd pitch TH + 1
//   C  R1  gx, gy on the TW x TH tile, row pitch TW + 1 (A is dead): K1x / K0x of B's arrays in
//          registers, four consecutive columns per thread
//   D       s, the diffusivity, the store; lanes run along x
// A staged position outside the image holds the value AT THE CLAMPED POSITION.  Every LDS index
// is tile-relative: B reads the rows [p - y0, p - y0 + 2 Ry] for the clamped row p in
// [y0, y0 + TH), C the columns [i, i + 2 Rx] for a tile column i < TW, both inside the staged
// tile for any image size (3 x 3 with halos longer than the axis included); tile positions
// outside the image are computed from the replicated border and never stored.
// A thread works on four outputs at a time, so one uniform tap load serves eight fma.  In B
// the four are the same column of four rows, lanes along the columns.  In C they are
// consecutive along x and share their input reads (W + 3 reads for 4 outputs instead of 4 W):
// output j takes input r with the tap r - j, read from a tap row padded with three zeros on
// either side, so each output still sums its taps t = -R..R in order and the zero taps add
// nothing; lanes run along the rows.  With B column-major every read of a wave is to
// consecutive addresses, and the odd pitches keep B's and C's transposing stores off a single
// bank.  D reads C's rows along x, so a wave's stores are 512 contiguous bytes per component.
// taps_y: [K0 | K1] of the axis; taps_xp: [0 0 0 K0 0 0 0 | 0 0 0 K1 0 0 0].
template <typename T, int MODE>
__global__ void __launch_bounds__(256) pm2_k(const double* __restrict__ in, const T* __restrict__ taps_xp,
                                             const T* __restrict__ taps_y, int Rx, int Ry, int nx,
                                             int ny, int TW, int TH, int S1, T ihx, T ihy, int64_t cs,
                                             double* __restrict__ D, double* __restrict__ gout,
                                             PmParams pp) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* R1 = reinterpret_cast<T*>(ved_smem);
  T* R2 = R1 + S1;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int WA = TW + 2 * Rx, HA = TH + 2 * Ry;  // staged image
  const int PB = TH + 1, PC = TW + 1;            // pitches of B (per column) and C (per row)
  const int Wx = 2 * Rx + 1, Wy = 2 * Ry + 1;
  const float iWA = 1.0f / (float)WA;
  // A: eight loads in flight per thread
  const int nA = WA * HA;
  for (int e0 = tid; e0 < nA; e0 += 2048) {
    double u[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = min(e0 + 256 * j, nA - 1);
      const int r = ced2_div(e, iWA), c = e - r * WA;
      const int yy = min(max(y0 - Ry + r, 0), ny - 1), xx = min(max(x0 - Rx + c, 0), nx - 1);
      u[j] = in[(int64_t)yy * nx + xx];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (e0 + 256 * j < nA) R1[e0 + 256 * j] = (T)u[j];
  }
  __syncthreads();
  // B: item = (staged column c, rows 4 g .. 4 g + 3); lanes run along c
  const int SB = WA * PB;
  for (int e = tid; e < WA * (TH / 4); e += 256) {
    const int g = ced2_div(e, iWA), c = e - g * WA;
    const T* a[4];
    T b0[4], b1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = min(y0 + 4 * g + j, ny - 1);
      a[j] = R1 + (p - y0) * WA + c;
      b0[j] = b1[j] = T(0);
    }
#pragma unroll 2
    for (int q = 0; q < Wy; ++q) {
      const T k0 = taps_y[q], k1 = taps_y[Wy + q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const T v = a[j][q * WA];
        b0[j] = fma(k0, v, b0[j]);
        b1[j] = fma(k1, v, b1[j]);
      }
    }
    T* o = R2 + c * PB + 4 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = b0[j];
      o[SB + j] = b1[j];
    }
  }
  __syncthreads();
  // C: item = (row rb, four consecutive tile columns i0..i0+3); lanes run along rb
  const int SC = TH * PC;
  const T* k0p = taps_xp;           // the padded taps: tap t at [3 + R + t]
  const T* k1p = taps_xp + Wx + 6;
  const float iTH = 1.0f / (float)TH;
  for (int e = tid; e < TH * (TW / 4); e += 256) {
    const int g = ced2_div(e, iTH), rb = e - g * TH, i0 = 4 * g;
    const T* c = R2 + i0 * PB + rb;
    T gx[4], gy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gx[j] = gy[j] = T(0);
#pragma unroll 2
    for (int r = 0; r < Wx + 3; ++r) {
      const T v0 = c[r * PB], v1 = c[SB + r * PB];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        gx[j] = fma(k1p[3 + r - j], v0, gx[j]);
        gy[j] = fma(k0p[3 + r - j], v1, gy[j]);
      }
    }
    T* o = R1 + rb * PC + i0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = gx[j] * ihx;
      o[SC + j] = gy[j] * ihy;
    }
  }
  __syncthreads();
  // D: one pixel per item; lanes run along x
  const int sh = __ffs(TW) - 1;
  for (int e = tid; e < TW * TH; e += 256) {
    const int xi = e & (TW - 1), o = e >> sh;
    const int i = x0 + xi, y = y0 + o;
    if (i >= nx || y >= ny) continue;
    const T gx = R1[o * PC + xi], gy = R1[SC + o * PC + xi];
    const int64_t p = (int64_t)y * nx + i;
    if (MODE == PM_GRADIENT) {
      D[p] = (double)gx;
      D[cs + p] = (double)gy;
      continue;
    }
    T s = gx * gx;
    s = s + gy * gy;
    if (MODE == PM_SQNORM) {
      reinterpret_cast<T*>(D)[p] = s;
      continue;
    }
    const double gv = pm_diffusivity((double)s, pp);
    D[p] = gv;
    D[cs + p] = 0.0;
    D[2 * cs + p] = gv;
    if (gout) gout[p] = gv;
  }
}

// ---------------------------------------------------------------------------------------
// Vector-valued images (mad_pm_desc.channels = C > 1; include/mad_pm.h "Vector-valued images"):
// one diffusivity from the summed squared gradients of all channels, s = s_0 + ... + s_{C-1},
// summed left to right in T.  The image is planar, channel c at element offset c N.  The scalar
// kernels above stay as they are (C = 1 launches them); the two below repeat their phases inside
// a channel loop rather than share code with them, so the scalar kernels' code does not move.
//
// 3D: ced_z_k and ced_y_k run per channel into three pass-2 volumes per channel, a = [a00_0,
// a10_0, a01_0, a00_1, ...] (each N elements); this x pass stages one channel's three rows at a
// time, keeps the voxel's running s in a register, and maps and stores once after the last
// channel: 3 C T in, 48 out (fp32 with the two passes before it: 48 C + 48 B per voxel, against
// 96 C for C scalar generations).  No thread leaves before the last barrier: a thread with
// i >= nx stages and waits with the others and skips the arithmetic and the stores.  The barrier
// at the head of channels 1.. keeps a channel's rows until every thread has read its taps.
// PM_GRADIENT: D = 3 C arrays, channel slowest, (gx, gy, gz) within a channel.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) pmv_x_k(const T* __restrict__ a, int C, int64_t N,
                                               const T* __restrict__ taps, int R, int nx, int ny, int nz,
                                               T ihx, T ihy, T ihz, int64_t cs, double* __restrict__ D,
                                               double* __restrict__ gout, PmParams pp) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* L = reinterpret_cast<T*>(ved_smem);
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * 256;
  const int i = x0 + tid;
  const bool live = i < nx;
  const int64_t row = ((int64_t)blockIdx.z * ny + blockIdx.y) * nx;
  const int64_t p = row + i;
  const int nw = 256 + 2 * R;
  const int W = 2 * R + 1;
  T s = T(0);
  for (int ch = 0; ch < C; ++ch) {
    const T* a00 = a + (int64_t)(3 * ch) * N;
    const T* a10 = a00 + N;
    const T* a01 = a10 + N;
    if (ch) __syncthreads();
    for (int e = tid; e < nw; e += 256) {
      const int64_t q = row + min(max(x0 - R + e, 0), nx - 1);
      L[e] = a00[q];
      L[nw + e] = a10[q];
      L[2 * nw + e] = a01[q];
    }
    __syncthreads();
    if (live) {
      const T* c = L + tid;
      T gx = T(0), gy = T(0), gz = T(0);
#pragma unroll 4
      for (int q = 0; q < W; ++q) {
        const T k0 = taps[q], k1 = taps[W + q];
        gx = fma(k1, c[q], gx);
        gy = fma(k0, c[nw + q], gy);
        gz = fma(k0, c[2 * nw + q], gz);
      }
      gx = gx * ihx;
      gy = gy * ihy;
      gz = gz * ihz;
      if (MODE == PM_GRADIENT) {
        double* G = D + (int64_t)(3 * ch) * cs;
        G[p] = (double)gx;
        G[cs + p] = (double)gy;
        G[2 * cs + p] = (double)gz;
      } else {
        T sc = gx * gx;
        sc = sc + gy * gy;
        sc = sc + gz * gz;
        s = ch ? s + sc : sc;
      }
    }
  }
  if (MODE == PM_GRADIENT || !live) return;
  if (MODE == PM_SQNORM) {
    reinterpret_cast<T*>(D)[p] = s;
    return;
  }
  const double g = pm_diffusivity((double)s, pp);
  D[p] = g;
  D[cs + p] = 0.0;
  D[2 * cs + p] = 0.0;
  D[3 * cs + p] = g;
  D[4 * cs + p] = 0.0;
  D[5 * cs + p] = g;
  if (gout) gout[p] = g;
}

// 2D: pm2_k's phases A-D inside a channel loop, on pm2_k's LDS regions (the same tile plan).  in
// holds C planes of N = nx ny pixels.  Phase D of a channel adds its s_c to the running s of the
// tile's pixels, which stays in registers: TW TH <= 2048 over 256 threads is at most
// PM2V_ACC = 8 pixels per thread, item e = tid + 256 j, in a loop of that compile-time bound.
// After the last channel the same items map and store: 8 C in, 24 out per pixel, against 32 C.
// Phase D of channel c reads gx, gy from R1, which phase A of channel c + 1 overwrites: the
// barrier at the head of channels 1.. stands between them.  PM_GRADIENT: D = 2 C arrays, channel
// slowest, (gx, gy) within a channel.
// Scalar registers: inside the loop every phase's tile constants would stay live over all four
// phases (the compiler hoists them out of the channel loop), about forty wave-uniform values
// over the kernel's arguments, more than the 102 scalar registers hold.  Each phase therefore
// derives its constants anew from opaque copies of (Rx, Ry, TW, TH) (pm_fresh), a few scalar
// instructions per phase and channel, and after the last channel the running s goes through
// each thread's own slots of R2 (dead by then) so that the map runs once, in a rolled loop.
enum { PM2V_ACC = 8 };

// a copy of a wave-uniform value the compiler cannot trace to its source: what is computed from
// it is computed where it stands, not hoisted out of the enclosing loop
__device__ inline int pm_fresh(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

template <typename T, int MODE>
__global__ void __launch_bounds__(256) pm2v_k(const double* __restrict__ in, int C, int64_t N,
                                              const T* __restrict__ taps_xp, const T* __restrict__ taps_y,
                                              int Rx, int Ry, int nx, int ny, int TW, int TH, int S1, T ihx,
                                              T ihy, int64_t cs, double* __restrict__ D,
                                              double* __restrict__ gout, PmParams pp) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* R1 = reinterpret_cast<T*>(ved_smem);
  T* R2 = R1 + S1;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  T s[PM2V_ACC];
#pragma unroll
  for (int j = 0; j < PM2V_ACC; ++j) s[j] = T(0);
  for (int ch = 0; ch < C; ++ch) {
    const double* u0 = in + (int64_t)ch * N;
    if (ch) __syncthreads();
    {  // A: eight loads in flight per thread
      const int rx = pm_fresh(Rx), ry = pm_fresh(Ry);
      const int WA = pm_fresh(TW) + 2 * rx, HA = pm_fresh(TH) + 2 * ry;  // staged image
      const float iWA = 1.0f / (float)WA;
      const int nA = WA * HA;
      for (int e0 = tid; e0 < nA; e0 += 2048) {
        double u[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int e = min(e0 + 256 * j, nA - 1);
          const int r = ced2_div(e, iWA), c = e - r * WA;
          const int yy = min(max(y0 - ry + r, 0), ny - 1), xx = min(max(x0 - rx + c, 0), nx - 1);
          u[j] = u0[(int64_t)yy * nx + xx];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (e0 + 256 * j < nA) R1[e0 + 256 * j] = (T)u[j];
      }
    }
    __syncthreads();
    {  // B: item = (staged column c, rows 4 g .. 4 g + 3); lanes run along c
      const int th = pm_fresh(TH);
      const int WA = pm_fresh(TW) + 2 * pm_fresh(Rx), PB = th + 1, Wy = 2 * pm_fresh(Ry) + 1;
      const float iWA = 1.0f / (float)WA;
      const int SB = WA * PB;
      for (int e = tid; e < WA * (th / 4); e += 256) {
        const int g = ced2_div(e, iWA), c = e - g * WA;
        const T* a[4];
        T b0[4], b1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int p = min(y0 + 4 * g + j, ny - 1);
          a[j] = R1 + (p - y0) * WA + c;
          b0[j] = b1[j] = T(0);
        }
#pragma unroll 2
        for (int q = 0; q < Wy; ++q) {
          const T k0 = taps_y[q], k1 = taps_y[Wy + q];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const T v = a[j][q * WA];
            b0[j] = fma(k0, v, b0[j]);
            b1[j] = fma(k1, v, b1[j]);
          }
        }
        T* o = R2 + c * PB + 4 * g;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = b0[j];
          o[SB + j] = b1[j];
        }
      }
    }
    __syncthreads();
    {  // C: item = (row rb, four consecutive tile columns i0..i0+3); lanes run along rb
      const int tw = pm_fresh(TW), th = pm_fresh(TH), rx = pm_fresh(Rx);
      const int PB = th + 1, PC = tw + 1, Wx = 2 * rx + 1;
      const int SB = (tw + 2 * rx) * PB, SC = th * PC;
      const T* k0p = taps_xp;  // the padded taps: tap t at [3 + R + t]
      const T* k1p = taps_xp + Wx + 6;
      const float iTH = 1.0f / (float)th;
      for (int e = tid; e < th * (tw / 4); e += 256) {
        const int g = ced2_div(e, iTH), rb = e - g * th, i0 = 4 * g;
        const T* c = R2 + i0 * PB + rb;
        T gx[4], gy[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) gx[j] = gy[j] = T(0);
#pragma unroll 2
        for (int r = 0; r < Wx + 3; ++r) {
          const T v0 = c[r * PB], v1 = c[SB + r * PB];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            gx[j] = fma(k1p[3 + r - j], v0, gx[j]);
            gy[j] = fma(k0p[3 + r - j], v1, gy[j]);
          }
        }
        T* o = R1 + rb * PC + i0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          o[j] = gx[j] * ihx;
          o[SC + j] = gy[j] * ihy;
        }
      }
    }
    __syncthreads();
    {  // D: one pixel per item; lanes run along x.  The channel's s_c joins the running s.
      const int tw = pm_fresh(TW), th = pm_fresh(TH);
      const int PC = tw + 1, SC = th * PC, sh = __ffs(tw) - 1, nD = tw * th;
#pragma unroll
      for (int j = 0; j < PM2V_ACC; ++j) {
        const int e = tid + 256 * j;
        if (e >= nD) continue;
        const int xi = e & (tw - 1), o = e >> sh;
        const T gx = R1[o * PC + xi], gy = R1[SC + o * PC + xi];
        if (MODE == PM_GRADIENT) {
          const int i = x0 + xi, y = y0 + o;
          if (i >= nx || y >= ny) continue;
          const int64_t p = (int64_t)y * nx + i;
          double* G = D + (int64_t)(2 * ch) * cs;
          G[p] = (double)gx;
          G[cs + p] = (double)gy;
          continue;
        }
        T sc = gx * gx;
        sc = sc + gy * gy;
        s[j] = ch ? s[j] + sc : sc;
      }
    }
  }
  if (MODE == PM_GRADIENT) return;
  // the map: each thread's s through its own slots of R2, last read by phase C before a barrier
  const int sh = __ffs(TW) - 1, nD = TW * TH;
#pragma unroll
  for (int j = 0; j < PM2V_ACC; ++j)
    if (tid + 256 * j < nD) R2[tid + 256 * j] = s[j];
  for (int e = tid; e < nD; e += 256) {
    const int xi = e & (TW - 1), o = e >> sh;
    const int i = x0 + xi, y = y0 + o;
    if (i >= nx || y >= ny) continue;
    const T sv = R2[e];
    const int64_t p = (int64_t)y * nx + i;
    if (MODE == PM_SQNORM) {
      reinterpret_cast<T*>(D)[p] = sv;
      continue;
    }
    const double gv = pm_diffusivity((double)sv, pp);
    D[p] = gv;
    D[cs + p] = 0.0;
    D[2 * cs + p] = gv;
    if (gout) gout[p] = gv;
  }
}

}  // namespace mad
