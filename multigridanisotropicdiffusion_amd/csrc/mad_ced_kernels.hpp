// mad_ced_kernels.hpp -- device kernels of the structure-tensor diffusion tensor
// (include/mad_ced.h): Weickert's edge- and coherence-enhancing diffusion.
//
// Five LDS-staged passes per tensor generation, in the style of the VED FIR passes
// (mad_ved_kernels.hpp): each pass stages its input lines once, runs the taps out of LDS and
// reads the taps with uniform (scalar) loads.  Storage and FIR arithmetic in T (fp32, or
// fp64 in MAD_FP64) with explicit fma and contraction off; the eigen-analysis, the
// eigenvalue map and the tensor are fp64 in every mode.
//   1. ced_z_k    image (fp64)        -> K0z u, K1z u                               8 + 2 T
//   2. ced_y_k    those two           -> K0y K0z u, K1y K0z u, K0y K1z u            2 T + 3 T
//   3. ced_x_k    those three         -> K0x(rho) of the six gradient products      3 T + 6 T
//                 (gradient and products live in LDS only)
//   4. ced_ry_k   six volumes         -> K0y(rho) of each                           6 T + 6 T
//   5. ced_rz_k   six volumes         -> K0z(rho) of each = J_rho, then per voxel   6 T + 48
//                 eigen-analysis, eigenvalue map, fp64 tensor (or J_rho itself)
// Algorithmic traffic in fp32: 16 + 20 + 36 + 48 + 72 = 192 B per voxel.
// 2D images take one fused kernel instead, ced2_k at the end of this file: 8 + 24 = 32 B per pixel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mad_ved_kernels.hpp"

namespace mad {

struct CedParams {
  int enhancement;  // MAD_CED_EED / MAD_CED_CED
  double k2;        // contrast^2
  double m;         // exponent
  double alpha;
};

template <typename T>
struct CedVol6 {
  T* v[6];
};

// z pass: o0 = K0z in, o1 = K1z in; taps [K0 | K1], each 2R + 1.  Block = 64 x 4 columns, ZT
// output planes; LDS holds the ZT + 2R input planes of the block's columns (fp64 -> T on the
// way in); each thread reads only its own column.
template <typename T>
__global__ void __launch_bounds__(256) ced_z_k(const double* __restrict__ in, T* __restrict__ o0,
                                               T* __restrict__ o1, const T* __restrict__ taps, int R,
                                               int nx, int ny, int nz, int ZT) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* L = reinterpret_cast<T*>(ved_smem);
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 64 + (tid & 63);
  const int j = blockIdx.y * 4 + (tid >> 6);
  const int z0 = blockIdx.z * ZT;
  const bool ok = i < nx && j < ny;
  const int64_t sz = (int64_t)nx * ny;
  const int64_t col = (int64_t)min(j, ny - 1) * nx + min(i, nx - 1);
  const int np = ZT + 2 * R;
  for (int m = 0; m < np; ++m) {
    const int kk = min(max(z0 - R + m, 0), nz - 1);
    L[m * 256 + tid] = (T)in[kk * sz + col];
  }
  const int W = 2 * R + 1;
  const int zend = min(ZT, nz - z0);
  for (int o = 0; o < zend; ++o) {
    T a0 = T(0), a1 = T(0);
    const T* c = L + o * 256 + tid;
#pragma unroll 4
    for (int q = 0; q < W; ++q) {
      const T v = c[q * 256];
      a0 = fma(taps[q], v, a0);
      a1 = fma(taps[W + q], v, a1);
    }
    if (ok) {
      const int64_t p = (int64_t)(z0 + o) * sz + col;
      o0[p] = a0;
      o1[p] = a1;
    }
  }
}

// y pass: a00 = K0y z0, a10 = K1y z0, a01 = K0y z1.  Block = 64 x-columns of one plane, YT
// output rows; LDS holds the YT + 2R input rows of both inputs.
template <typename T>
__global__ void __launch_bounds__(256) ced_y_k(const T* __restrict__ z0, const T* __restrict__ z1,
                                               T* __restrict__ a00, T* __restrict__ a10,
                                               T* __restrict__ a01, const T* __restrict__ taps, int R,
                                               int nx, int ny, int nz, int YT) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* L = reinterpret_cast<T*>(ved_smem);
  const int tid = threadIdx.x;
  const int xi = tid & 63;
  const int i = blockIdx.x * 64 + xi;
  const int y0 = blockIdx.y * YT;
  const int k = blockIdx.z;
  const int64_t sz = (int64_t)nx * ny;
  const int64_t pl = (int64_t)k * sz + min(i, nx - 1);
  const int nr = YT + 2 * R;
  const int S2 = nr * 64;  // one input's slab in LDS
  for (int r = tid >> 6; r < nr; r += 4) {
    const int jj = min(max(y0 - R + r, 0), ny - 1);
    const int64_t q = pl + (int64_t)jj * nx;
    L[r * 64 + xi] = z0[q];
    L[S2 + r * 64 + xi] = z1[q];
  }
  __syncthreads();
  if (i >= nx) return;
  const int W = 2 * R + 1;
  const int yend = min(YT, ny - y0);
  for (int o = tid >> 6; o < yend; o += 4) {
    T s00 = T(0), s10 = T(0), s01 = T(0);
    const T* c = L + o * 64 + xi;
#pragma unroll 4
    for (int q = 0; q < W; ++q) {
      const T v0 = c[q * 64], v1 = c[S2 + q * 64];
      const T k0 = taps[q], k1 = taps[W + q];
      s00 = fma(k0, v0, s00);
      s10 = fma(k1, v0, s10);
      s01 = fma(k0, v1, s01);
    }
    const int64_t p = pl + (int64_t)(y0 + o) * nx;
    a00[p] = s00;
    a10[p] = s10;
    a01[p] = s01;
  }
}

// x pass fused with the products and the rho smoothing along x.  Block = 256 consecutive x of
// one row.  LDS: the three input rows over [x0 - Rs - Rr, x0 + 256 + Rs + Rr) (clamped), then
// the six products over [x0 - Rr, x0 + 256 + Rr), taken at the CLAMPED positions (the rho
// pass's clamp acts on the product volumes, so the halo repeats the edge voxel's products).
// taps_s = [K0 | K1] of sigma (2 Rs + 1 each), taps_r = K0 of rho (2 Rr + 1).
// ih = (1 / hx, 1 / hy, 1 / hz), each applied once to its gradient component.
template <typename T>
__global__ void __launch_bounds__(256) ced_x_k(const T* __restrict__ a00, const T* __restrict__ a10,
                                               const T* __restrict__ a01, CedVol6<T> out,
                                               const T* __restrict__ taps_s, int Rs,
                                               const T* __restrict__ taps_r, int Rr, int nx, int ny,
                                               int nz, T ihx, T ihy, T ihz) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* L = reinterpret_cast<T*>(ved_smem);
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * 256;
  const int i = x0 + tid;
  const int j = blockIdx.y;
  const int k = blockIdx.z;
  const int64_t row = ((int64_t)k * ny + j) * nx;
  const int nw = 256 + 2 * (Rs + Rr);  // staged inputs
  const int ng = 256 + 2 * Rr;         // gradient / product positions
  T* P = L + 3 * nw;                   // six product rows of ng
  const int xs = x0 - Rs - Rr;         // x of staged element 0
  for (int e = tid; e < nw; e += 256) {
    const int64_t q = row + min(max(xs + e, 0), nx - 1);
    L[e] = a00[q];
    L[nw + e] = a10[q];
    L[2 * nw + e] = a01[q];
  }
  __syncthreads();
  const int Ws = 2 * Rs + 1;
  for (int m = tid; m < ng; m += 256) {
    // gradient at the clamped position p; its taps reach [p - Rs, p + Rs], inside the staged
    // range because p lies in [x0 - Rr, x0 + 255 + Rr]
    const int p = min(max(x0 - Rr + m, 0), nx - 1);
    const T* c = L + (p - xs - Rs);
    T gx = T(0), gy = T(0), gz = T(0);
#pragma unroll 4
    for (int q = 0; q < Ws; ++q) {
      const T k0 = taps_s[q], k1 = taps_s[Ws + q];
      gx = fma(k1, c[q], gx);
      gy = fma(k0, c[nw + q], gy);
      gz = fma(k0, c[2 * nw + q], gz);
    }
    gx = gx * ihx;
    gy = gy * ihy;
    gz = gz * ihz;
    P[m] = gx * gx;
    P[ng + m] = gx * gy;
    P[2 * ng + m] = gx * gz;
    P[3 * ng + m] = gy * gy;
    P[4 * ng + m] = gy * gz;
    P[5 * ng + m] = gz * gz;
  }
  __syncthreads();
  if (i >= nx) return;
  const int Wr = 2 * Rr + 1;
  T s0 = T(0), s1 = T(0), s2 = T(0), s3 = T(0), s4 = T(0), s5 = T(0);
  const T* c = P + tid;
#pragma unroll 4
  for (int q = 0; q < Wr; ++q) {
    const T kr = taps_r[q];
    s0 = fma(kr, c[q], s0);
    s1 = fma(kr, c[ng + q], s1);
    s2 = fma(kr, c[2 * ng + q], s2);
    s3 = fma(kr, c[3 * ng + q], s3);
    s4 = fma(kr, c[4 * ng + q], s4);
    s5 = fma(kr, c[5 * ng + q], s5);
  }
  const int64_t p = row + i;
  out.v[0][p] = s0;
  out.v[1][p] = s1;
  out.v[2][p] = s2;
  out.v[3][p] = s3;
  out.v[4][p] = s4;
  out.v[5][p] = s5;
}

// rho smoothing along y of the six volumes.  Block = 64 x-columns of one plane, YT output
// rows; LDS holds the YT + 2R rows of one volume at a time.
template <typename T>
__global__ void __launch_bounds__(256) ced_ry_k(CedVol6<const T> in, CedVol6<T> out,
                                                const T* __restrict__ taps, int R, int nx, int ny,
                                                int nz, int YT) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* L = reinterpret_cast<T*>(ved_smem);
  const int tid = threadIdx.x;
  const int xi = tid & 63;
  const int i = blockIdx.x * 64 + xi;
  const int y0 = blockIdx.y * YT;
  const int k = blockIdx.z;
  const int64_t sz = (int64_t)nx * ny;
  const int64_t pl = (int64_t)k * sz + min(i, nx - 1);
  const int nr = YT + 2 * R;
  const int W = 2 * R + 1;
  const int yend = min(YT, ny - y0);
  for (int v = 0; v < 6; ++v) {
    const T* __restrict__ src = in.v[v];
    T* __restrict__ dst = out.v[v];
    if (v) __syncthreads();  // the previous volume's rows are consumed
    for (int r = tid >> 6; r < nr; r += 4) {
      const int jj = min(max(y0 - R + r, 0), ny - 1);
      L[r * 64 + xi] = src[pl + (int64_t)jj * nx];
    }
    __syncthreads();
    if (i < nx) {
      for (int o = tid >> 6; o < yend; o += 4) {
        T s = T(0);
        const T* c = L + o * 64 + xi;
#pragma unroll 4
        for (int q = 0; q < W; ++q) s = fma(taps[q], c[q * 64], s);
        dst[pl + (int64_t)(y0 + o) * nx] = s;
      }
    }
  }
}

// h(d) = exp(-(K^2 / d)^m) for d > 0, 0 otherwise
__device__ inline double ced_stop(double d, const CedParams& cp) {
  return d > 0.0 ? exp(-pow(cp.k2 / d, cp.m)) : 0.0;
}

enum { CED_TENSOR = 0, CED_STRUCTURE = 1 };

// one voxel: J_rho out (CED_STRUCTURE, fp64 SoA with component stride cs), or the
// eigen-analysis (cyclic Jacobi in fp64), the eigenvalue map and D = sum lam_i v_i v_i^T
// (CED_TENSOR; lam: optional three volumes of the mapped eigenvalues, stride n)
template <int MODE>
__device__ __forceinline__ void ced_point(double J0, double J1, double J2, double J3, double J4,
                                          double J5, int64_t p, int64_t cs, double* __restrict__ D,
                                          double* __restrict__ lam, int64_t n, const CedParams& cp) {
#pragma clang fp contract(off)
  if (MODE == CED_STRUCTURE) {
    D[p] = J0;
    D[cs + p] = J1;
    D[2 * cs + p] = J2;
    D[3 * cs + p] = J3;
    D[4 * cs + p] = J4;
    D[5 * cs + p] = J5;
    return;
  }
  double w[3], V[3][3], l[3];
  sym3_eigen<double>(J0, J1, J2, J3, J4, J5, w, V);
  const double oma = 1.0 - cp.alpha;
  if (cp.enhancement == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) l[q] = 1.0 - oma * ced_stop(w[q] - w[0], cp);
  } else {
#pragma unroll
    for (int q = 0; q < 3; ++q) l[q] = cp.alpha + oma * ced_stop(w[2] - w[q], cp);
  }
  double d[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const double a = l[q] * V[0][q], b = l[q] * V[1][q], c = l[q] * V[2][q];
    d[0] += a * V[0][q];
    d[1] += a * V[1][q];
    d[2] += a * V[2][q];
    d[3] += b * V[1][q];
    d[4] += b * V[2][q];
    d[5] += c * V[2][q];
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) D[q * cs + p] = d[q];
  if (lam) {
    lam[p] = l[0];
    lam[n + p] = l[1];
    lam[2 * n + p] = l[2];
  }
}

// rho smoothing along z of the six volumes, fused with ced_point.  Block = 64 x-columns of
// one row, ZT output planes shared by the block's four waves; LDS holds the ZT + 2R input
// planes of the six volumes over the block's columns.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) ced_rz_k(CedVol6<const T> in, const T* __restrict__ taps, int R,
                                                int nx, int ny, int nz, int ZT, int64_t cs,
                                                double* __restrict__ D, double* __restrict__ lam,
                                                CedParams cp) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* L = reinterpret_cast<T*>(ved_smem);
  const int tid = threadIdx.x;
  const int xi = tid & 63;
  const int i = blockIdx.x * 64 + xi;
  const int j = blockIdx.y;
  const int z0 = blockIdx.z * ZT;
  const int64_t sz = (int64_t)nx * ny;
  const int64_t col = (int64_t)j * nx + min(i, nx - 1);
  const int np = ZT + 2 * R;
  const int S6 = np * 64;  // one volume's slab in LDS
  for (int r = tid >> 6; r < np; r += 4) {
    const int kk = min(max(z0 - R + r, 0), nz - 1);
    const int64_t q = (int64_t)kk * sz + col;
#pragma unroll
    for (int v = 0; v < 6; ++v) L[v * S6 + r * 64 + xi] = in.v[v][q];
  }
  __syncthreads();
  if (i >= nx) return;
  const int W = 2 * R + 1;
  const int zend = min(ZT, nz - z0);
  const int64_t n = sz * nz;
  for (int o = tid >> 6; o < zend; o += 4) {
    T s0 = T(0), s1 = T(0), s2 = T(0), s3 = T(0), s4 = T(0), s5 = T(0);
    const T* c = L + o * 64 + xi;
#pragma unroll 4
    for (int q = 0; q < W; ++q) {
      const T kr = taps[q];
      s0 = fma(kr, c[q * 64], s0);
      s1 = fma(kr, c[S6 + q * 64], s1);
      s2 = fma(kr, c[2 * S6 + q * 64], s2);
      s3 = fma(kr, c[3 * S6 + q * 64], s3);
      s4 = fma(kr, c[4 * S6 + q * 64], s4);
      s5 = fma(kr, c[5 * S6 + q * 64], s5);
    }
    ced_point<MODE>((double)s0, (double)s1, (double)s2, (double)s3, (double)s4, (double)s5,
                    (int64_t)(z0 + o) * sz + col, cs, D, lam, n, cp);
  }
}

// ---------------------------------------------------------------------------------------
// 2D: one fused kernel per tensor generation (include/mad_ced.h "2D").  The sigma + rho halo
// of a 2D tile fits LDS, so the image goes in and the fp64 tensor comes out with nothing in
// between touching memory: 8 + 24 = 32 algorithmic bytes per pixel.

// h(t) as ced_stop; the default exponent 2 (and 1) skips pow
__device__ inline double ced2_stop(double t, const CedParams& cp) {
#pragma clang fp contract(off)
  if (!(t > 0.0)) return 0.0;
  const double x = cp.k2 / t;
  return exp(-(cp.m == 2.0 ? x * x : cp.m == 1.0 ? x : pow(x, cp.m)));
}

// floor(e / W) for 0 <= e < 2^20 from inv = 1.0f / W: (e + 0.5) / W is at least 0.5 / W away from
// an integer, the two roundings move it by less than e / W * 2^-23
__device__ __forceinline__ int ced2_div(int e, float inv) { return (int)(((float)e + 0.5f) * inv); }

// one pixel: J_rho = [[a, b], [b, c]] out (CED_STRUCTURE), or the closed-form eigenvalues
// mu = m -+ r, the eigenvalue map on mu1 - mu0 = 2 r, and D = s I + q [[d, b], [b, -d]]
// (= sum lam_i v_i v_i^T without eigenvectors, continuous at r = 0); lam: optional two
// arrays of the mapped eigenvalues, stride n.  fp64 in every mode.
template <int MODE>
__device__ __forceinline__ void ced2_point(double a, double b, double c, int64_t p, int64_t cs,
                                           double* __restrict__ D, double* __restrict__ lam,
                                           int64_t n, const CedParams& cp) {
#pragma clang fp contract(off)
  if (MODE == CED_STRUCTURE) {
    D[p] = a;
    D[cs + p] = b;
    D[2 * cs + p] = c;
    return;
  }
  const double d = 0.5 * (a - c);
  const double r = hypot(d, b);
  const double h = (1.0 - cp.alpha) * ced2_stop(2.0 * r, cp);
  double l0, l1;
  if (cp.enhancement == 0) {
    l0 = 1.0;
    l1 = 1.0 - h;
  } else {
    l0 = cp.alpha + h;
    l1 = cp.alpha;
  }
  const double s = 0.5 * (l0 + l1);
  const double q = r > 0.0 ? (l1 - l0) / (2.0 * r) : 0.0;
  const double qd = q * d;
  D[p] = s + qd;
  D[cs + p] = q * b;
  D[2 * cs + p] = s - qd;
  if (lam) {
    lam[p] = l0;
    lam[n + p] = l1;
  }
}

// Block = 256 threads, a TW x TH output tile at (x0, y0); TW a power of two, TH a multiple of 4.
// With H = Rs + Rr per axis, LDS holds two regions that the phases use in turn (S1 = the size of
// the first in elements, from the host):
//   A  R1  image tile (TW + 2 Hx) x (TH + 2 Hy), clamped, fp64 -> T
//   B  R2  K0y u, K1y u at the rows clamp(y0 - Rr_y + rb), rb < HB = TH + 2 Rr_y, all staged columns
//   C  R1  gx gx, gx gy, gy gy at the columns clamp(x0 - Rr_x + m) of those rows (A is dead),
//          stored column-major with the odd pitch HB + 1
//   D  R2  K0x(rho) of the three on the TW tile columns, same rows, row pitch TW + 1 (B is dead)
//   E       K0y(rho) in registers, ced2_point, store
// A halo position outside the image holds the value AT THE CLAMPED POSITION (each pass's clamp
// acts on the previous pass's output, as in the 3D kernels).  Every LDS index is tile-relative
// and built from a clamped coordinate p with x0 - Rr <= p <= x0 + TW - 1 + Rr (the tile starts
// inside the image), so p +- Rs stays inside the staged range for any image size.
// A thread works on four outputs at a time, so one uniform tap load serves eight (B, C) or
// twelve (D, E) fma, their LDS reads are in flight together and the index arithmetic is paid
// once per four.  In B and C the four are the same column of four rows.  In D and E they are
// consecutive along the filtered axis and share their input reads (W + 3 reads for 4 outputs
// instead of 4 W): output j takes input r with the tap r - j, read from a tap row padded with
// three zeros on either side, so each output still sums its taps t = -R..R in order and the
// zero taps add nothing.  With the column-major products a wave's lanes run along the rows in
// D and along x in E: both read consecutive addresses, and the odd pitches keep C's and D's
// transposing stores off a single bank.
// taps_x / taps_y: [K0(sigma) | K1(sigma) | 0 0 0 K0(rho) 0 0 0] of the axis.
template <typename T, int MODE>
__global__ void __launch_bounds__(256) ced2_k(const double* __restrict__ in, const T* __restrict__ taps_x,
                                              const T* __restrict__ taps_y, int Rsx, int Rsy, int Rrx,
                                              int Rry, int nx, int ny, int TW, int TH, int S1, T ihx,
                                              T ihy, int64_t cs, double* __restrict__ D,
                                              double* __restrict__ lam, CedParams cp) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char ved_smem[];
  T* R1 = reinterpret_cast<T*>(ved_smem);
  T* R2 = R1 + S1;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int Hx = Rsx + Rrx, Hy = Rsy + Rry;
  const int WA = TW + 2 * Hx, HA = TH + 2 * Hy;  // staged image
  const int HB = TH + 2 * Rry;                   // rows of phases B, C, D
  const int WC = TW + 2 * Rrx;                   // columns of phase C
  const int PC = HB + 1, PD = TW + 1;            // pitches of C (per column) and D (per row)
  const int Wsx = 2 * Rsx + 1, Wsy = 2 * Rsy + 1, Wrx = 2 * Rrx + 1, Wry = 2 * Rry + 1;
  const float iWA = 1.0f / (float)WA, iWC = 1.0f / (float)WC;
  // A: eight loads in flight per thread
  const int nA = WA * HA;
  for (int e0 = tid; e0 < nA; e0 += 2048) {
    double u[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int e = min(e0 + 256 * j, nA - 1);
      const int r = ced2_div(e, iWA), c = e - r * WA;
      const int yy = min(max(y0 - Hy + r, 0), ny - 1), xx = min(max(x0 - Hx + c, 0), nx - 1);
      u[j] = in[(int64_t)yy * nx + xx];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (e0 + 256 * j < nA) R1[e0 + 256 * j] = (T)u[j];
  }
  __syncthreads();
  // B: item = (staged column c, rows 4 g .. 4 g + 3); lanes run along c
  const int nB = WA * HB, GB = (HB + 3) / 4;
  for (int e = tid; e < WA * GB; e += 256) {
    const int g = ced2_div(e, iWA), c = e - g * WA;
    const T* a[4];
    T b0[4], b1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = min(max(y0 - Rry + min(4 * g + j, HB - 1), 0), ny - 1);
      a[j] = R1 + (p - Rsy - (y0 - Hy)) * WA + c;
      b0[j] = b1[j] = T(0);
    }
#pragma unroll 2
    for (int q = 0; q < Wsy; ++q) {
      const T k0 = taps_y[q], k1 = taps_y[Wsy + q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const T v = a[j][q * WA];
        b0[j] = fma(k0, v, b0[j]);
        b1[j] = fma(k1, v, b1[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * g + j < HB) {
        R2[(4 * g + j) * WA + c] = b0[j];
        R2[nB + (4 * g + j) * WA + c] = b1[j];
      }
  }
  __syncthreads();
  // C: item = (product column m, rows 4 g .. 4 g + 3); lanes run along m
  const int SC = WC * PC;
  for (int e = tid; e < WC * GB; e += 256) {
    const int g = ced2_div(e, iWC), m = e - g * WC;
    const int p = min(max(x0 - Rrx + m, 0), nx - 1);
    const T* b[4];
    T gx[4], gy[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[j] = R2 + min(4 * g + j, HB - 1) * WA + (p - Rsx - (x0 - Hx));
      gx[j] = gy[j] = T(0);
    }
#pragma unroll 2
    for (int q = 0; q < Wsx; ++q) {
      const T k0 = taps_x[q], k1 = taps_x[Wsx + q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        gx[j] = fma(k1, b[j][q], gx[j]);
        gy[j] = fma(k0, b[j][nB + q], gy[j]);
      }
    }
    T* o = R1 + m * PC + 4 * g;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * g + j < HB) {
        const T x = gx[j] * ihx, y = gy[j] * ihy;
        o[j] = x * x;
        o[SC + j] = x * y;
        o[2 * SC + j] = y * y;
      }
  }
  __syncthreads();
  // D: item = (row rb, four consecutive tile columns i0..i0+3); lanes run along rb
  const int SD = HB * PD;
  const T* krx = taps_x + 2 * Wsx;  // the padded rho taps: tap t at [3 + t]
  const float iHB = 1.0f / (float)HB;
  for (int e = tid; e < HB * (TW / 4); e += 256) {
    const int g = ced2_div(e, iHB), rb = e - g * HB, i0 = 4 * g;
    const T* c = R1 + i0 * PC + rb;
    T s[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[a][j] = T(0);
#pragma unroll 2
    for (int r = 0; r < Wrx + 3; ++r) {
      const T v0 = c[r * PC], v1 = c[SC + r * PC], v2 = c[2 * SC + r * PC];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const T kr = krx[3 + r - j];
        s[0][j] = fma(kr, v0, s[0][j]);
        s[1][j] = fma(kr, v1, s[1][j]);
        s[2][j] = fma(kr, v2, s[2][j]);
      }
    }
    T* o = R2 + rb * PD + i0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) o[a * SD + j] = s[a][j];
  }
  __syncthreads();
  // E: item = (tile column xi, four consecutive rows o..o+3); lanes run along x
  const int yend = min(TH, ny - y0);
  const T* kry = taps_y + 2 * Wsy;
  const int64_t n = (int64_t)nx * ny;
  for (int e = tid; e < TW * (TH / 4); e += 256) {
    const int xi = e & (TW - 1), o = 4 * (e / TW), i = x0 + xi;
    if (i >= nx) continue;
    const T* c = R2 + o * PD + xi;
    T s[3][4];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[a][j] = T(0);
#pragma unroll 2
    for (int r = 0; r < Wry + 3; ++r) {
      const T v0 = c[r * PD], v1 = c[SD + r * PD], v2 = c[2 * SD + r * PD];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const T kr = kry[3 + r - j];
        s[0][j] = fma(kr, v0, s[0][j]);
        s[1][j] = fma(kr, v1, s[1][j]);
        s[2][j] = fma(kr, v2, s[2][j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (o + j < yend)
        ced2_point<MODE>((double)s[0][j], (double)s[1][j], (double)s[2][j], (int64_t)(y0 + o + j) * nx + i, cs,
                         D, lam, n, cp);
  }
}

}  // namespace mad
