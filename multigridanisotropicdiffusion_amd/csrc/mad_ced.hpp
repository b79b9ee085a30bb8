// mad_ced.hpp -- host driver + C ABI of include/mad_ced.h (structure-tensor EED / CED on the
// GPU).  Included at the end of mad_solver.hip, after mad_ved.hpp: like the VED driver it
// hands the device tensor to the MAD solver in place (tensor_at0) and runs the diffusion
// steps through run_impl, no host round trips between tensor generation and solve.
#include "../../include/mad_ced.h"
#include "mad_ced_kernels.hpp"

struct mad_ced_ctx {
  mad_ced_desc d{};
  std::string err;
  mad_ctx* mad = nullptr;  // the diffusion solver, kept across iterations
  int dim = 3;             // 2: the fused kernel ced2_k, tensor [xx,xy,yy]
  int tile[2] = {0, 0};    // 2D: the output tile of the last tensor generation (x, y)
  int64_t n[3] = {0, 0, 0};
  int64_t N = 0;
  double* img = nullptr;   // internal image (fp64)
  double* img2 = nullptr;  // next iterate
  void* vol = nullptr;     // 12 scratch volumes in the storage precision
  void* taps = nullptr;    // device taps, per axis [K0(sigma) | K1(sigma) | K0(rho)] (2D: K0(rho) zero-padded)
  int Rs[3] = {0, 0, 0}, Rr[3] = {0, 0, 0};
  size_t tap_off[3] = {0, 0, 0};  // element offset of each axis' taps
  double* lam = nullptr;   // mapped eigenvalues, SoA x3 (mad_ced_tensor only)
  void* stage = nullptr;   // host <-> device staging
  size_t stage_bytes = 0;
  ~mad_ced_ctx() {
    if (mad) (void)hipSetDevice(mad->device);
    if (mad && mad->stream) (void)hipStreamSynchronize(mad->stream);
    for (void* p : {(void*)img, (void*)img2, vol, taps, (void*)lam, stage})
      if (p) (void)hipFree(p);
    if (mad) mad_destroy(mad);
  }
};

namespace {

template <typename F>
int ced_guarded(mad_ced_ctx* v, F&& f) {
  try {
    f();
    return MAD_OK;
  } catch (const MadError& e) {
    g_last_error = e.what();
    if (v) v->err = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    g_last_error = "out of host memory";
    if (v) v->err = g_last_error;
    return MAD_ERR_NOMEM;
  } catch (const std::exception& e) {
    g_last_error = e.what();
    if (v) v->err = e.what();
    return MAD_ERR_DEVICE;
  }
}

void* ced_stage(mad_ced_ctx* v, size_t bytes) {
  if (bytes > v->stage_bytes) {
    if (v->stage) HIP_CHECK(hipFree(v->stage));
    v->stage = nullptr;
    v->stage_bytes = 0;
    HIP_CHECK(hipMalloc(&v->stage, bytes));
    v->stage_bytes = bytes;
  }
  return v->stage;
}

// host or device image (any dtype) -> v->img (fp64)
void ced_load_image(mad_ced_ctx* v, const void* src, int dt, bool dev) {
  const size_t es = dtype_size(dt);
  REQUIRE(es, MAD_ERR_INVALID, "bad image dtype");
  hipStream_t st = v->mad->stream;
  if (!dev) {
    void* s = ced_stage(v, es * v->N);
    HIP_CHECK(hipMemcpyAsync(s, src, es * v->N, hipMemcpyHostToDevice, st));
    src = s;
  }
  convert_to<double>(src, dt, v->img, v->N, st);
}

// allow the passes more than the default 64 KiB of dynamic LDS (once per type)
template <typename T>
void ced_lds_attr() {
  static bool done = false;
  if (done) return;
  for (const void* k : {(const void*)ced_z_k<T>, (const void*)ced_y_k<T>, (const void*)ced_x_k<T>,
                        (const void*)ced_ry_k<T>, (const void*)ced_rz_k<T, CED_TENSOR>,
                        (const void*)ced_rz_k<T, CED_STRUCTURE>})
    HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVedLds));
  done = true;
}

template <typename T>
void ced2_lds_attr() {
  static bool done = false;
  if (done) return;
  for (const void* k : {(const void*)ced2_k<T, CED_TENSOR>, (const void*)ced2_k<T, CED_STRUCTURE>})
    HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVedLds));
  done = true;
}

// the taps of both scales on every axis (ved_taps: the VED FIR operator's K0, K1), in the
// storage precision, uploaded once: the scales are fixed for the context's lifetime.  2D: three
// zeros on either side of K0(rho), for ced2_k's four-outputs-per-thread rho phases.
template <typename T>
void ced_upload_taps(mad_ced_ctx* v) {
  std::vector<T> kt;
  const int pad = v->dim == 2 ? 3 : 0;
  for (int q = 0; q < v->dim; ++q) {
    std::vector<double> Ks, Kr;
    v->Rs[q] = ved_taps(v->d.noise_scale, v->d.spacing[q], Ks);
    v->Rr[q] = ved_taps(v->d.feature_scale, v->d.spacing[q], Kr);
    const int Ws = 2 * v->Rs[q] + 1, Wr = 2 * v->Rr[q] + 1;
    v->tap_off[q] = kt.size();
    for (int t = 0; t < 2 * Ws; ++t) kt.push_back((T)Ks[t]);  // K0 | K1
    kt.insert(kt.end(), pad, T(0));
    for (int t = 0; t < Wr; ++t) kt.push_back((T)Kr[t]);      // K0
    kt.insert(kt.end(), pad, T(0));
  }
  HIP_CHECK(hipMalloc(&v->taps, sizeof(T) * kt.size()));
  HIP_CHECK(hipMemcpy(v->taps, kt.data(), sizeof(T) * kt.size(), hipMemcpyHostToDevice));
}

// One tensor generation from v->img: the five passes of mad_ced_kernels.hpp.  mode
// CED_TENSOR: D = the tensor (component stride cs), lam optional; CED_STRUCTURE: D = J_rho.
// ev: six events around the passes (may be null).
template <typename T>
void ced_generate(mad_ced_ctx* v, int mode, double* D, int64_t cs, double* lam, Event* ev) {
  hipStream_t st = v->mad->stream;
  const int nx = (int)v->n[0], ny = (int)v->n[1], nz = (int)v->n[2];
  const int64_t N = v->N;
  if (!v->vol) HIP_CHECK(big_alloc((void**)&v->vol, sizeof(T) * 12 * N));
  T* f = (T*)v->vol;
  // slots: pass 1 -> 0, 1; pass 2 -> 2..4; pass 3 -> 6..11; pass 4 -> 0..5 (1, 2 outputs dead)
  T *z0 = f, *z1 = f + N, *a00 = f + 2 * N, *a10 = f + 3 * N, *a01 = f + 4 * N;
  CedVol6<T> X, Y;
  CedVol6<const T> Xc, Yc;
  for (int q = 0; q < 6; ++q) {
    Xc.v[q] = X.v[q] = f + (6 + q) * N;
    Yc.v[q] = Y.v[q] = f + q * N;
  }
  const T* tp = (const T*)v->taps;
  const int* Rs = v->Rs;
  const int* Rr = v->Rr;
  const T *sx = tp + v->tap_off[0], *sy = tp + v->tap_off[1], *sz_ = tp + v->tap_off[2];
  const T *rx = sx + 2 * (2 * Rs[0] + 1), *ry = sy + 2 * (2 * Rs[1] + 1), *rz = sz_ + 2 * (2 * Rs[2] + 1);
  // tiles: z / y tiles shrink with long taps (as ved_scale's); the x row is 256 wide
  auto lds_for = [](int lines, int width, int copies) { return (size_t)lines * width * copies * sizeof(T); };
  int ZT = 32, YT = 32, YR = 32, ZR = 32;
  while (ZT > 4 && lds_for(ZT + 2 * Rs[2], 256, 1) > kVedLds) ZT /= 2;
  while (YT > 4 && lds_for(YT + 2 * Rs[1], 64, 2) > kVedLds) YT /= 2;
  while (YR > 4 && lds_for(YR + 2 * Rr[1], 64, 1) > kVedLds) YR /= 2;
  // the last pass holds six volumes' planes: tiles of <= 64 KiB keep two blocks on a CU
  while (ZR > 8 && lds_for(ZR + 2 * Rr[2], 64, 6) > 64 * 1024) ZR /= 2;
  while (ZR > 4 && lds_for(ZR + 2 * Rr[2], 64, 6) > kVedLds) ZR /= 2;
  const size_t l1 = lds_for(ZT + 2 * Rs[2], 256, 1), l2 = lds_for(YT + 2 * Rs[1], 64, 2);
  const size_t l3 = lds_for(256 + 2 * (Rs[0] + Rr[0]), 1, 3) + lds_for(256 + 2 * Rr[0], 1, 6);
  const size_t l4 = lds_for(YR + 2 * Rr[1], 64, 1), l5 = lds_for(ZR + 2 * Rr[2], 64, 6);
  REQUIRE(l1 <= kVedLds && l2 <= kVedLds && l3 <= kVedLds && l4 <= kVedLds && l5 <= kVedLds,
          MAD_ERR_UNSUPPORTED, "Gaussian taps too long for the LDS tiles (scale / spacing too large)");
  ced_lds_attr<T>();
  const double* h = v->d.spacing;
  const CedParams cp{v->d.enhancement, v->d.contrast * v->d.contrast, v->d.exponent, v->d.alpha};
  if (ev) HIP_CHECK(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL((ced_z_k<T>), dim3((nx + 63) / 64, (ny + 3) / 4, (nz + ZT - 1) / ZT), dim3(256), l1, st,
                     v->img, z0, z1, sz_, Rs[2], nx, ny, nz, ZT);
  if (ev) HIP_CHECK(hipEventRecord(ev[1], st));
  hipLaunchKernelGGL((ced_y_k<T>), dim3((nx + 63) / 64, (ny + YT - 1) / YT, nz), dim3(256), l2, st, z0, z1,
                     a00, a10, a01, sy, Rs[1], nx, ny, nz, YT);
  if (ev) HIP_CHECK(hipEventRecord(ev[2], st));
  hipLaunchKernelGGL((ced_x_k<T>), dim3((nx + 255) / 256, ny, nz), dim3(256), l3, st, a00, a10, a01, X, sx,
                     Rs[0], rx, Rr[0], nx, ny, nz, (T)(1.0 / h[0]), (T)(1.0 / h[1]), (T)(1.0 / h[2]));
  if (ev) HIP_CHECK(hipEventRecord(ev[3], st));
  hipLaunchKernelGGL((ced_ry_k<T>), dim3((nx + 63) / 64, (ny + YR - 1) / YR, nz), dim3(256), l4, st, Xc, Y,
                     ry, Rr[1], nx, ny, nz, YR);
  if (ev) HIP_CHECK(hipEventRecord(ev[4], st));
  const dim3 g5((nx + 63) / 64, ny, (nz + ZR - 1) / ZR);
  if (mode == CED_STRUCTURE)
    hipLaunchKernelGGL((ced_rz_k<T, CED_STRUCTURE>), g5, dim3(256), l5, st, Yc, rz, Rr[2], nx, ny, nz, ZR, cs,
                       D, nullptr, cp);
  else
    hipLaunchKernelGGL((ced_rz_k<T, CED_TENSOR>), g5, dim3(256), l5, st, Yc, rz, Rr[2], nx, ny, nz, ZR, cs, D,
                       lam, cp);
  if (ev) HIP_CHECK(hipEventRecord(ev[5], st));
  HIP_CHECK(hipGetLastError());
}

// The LDS regions of ced2_k for a TW x TH tile, in elements: R1 = image tile | three products
// (column-major, pitch HB + 1), R2 = K0y u, K1y u | three x-smoothed products (row pitch TW + 1);
// the kernel's comment names the phases.
struct Ced2Lds {
  int s1, s2;
};
Ced2Lds ced2_lds(int TW, int TH, const int* Rs, const int* Rr) {
  const int WA = TW + 2 * (Rs[0] + Rr[0]), HA = TH + 2 * (Rs[1] + Rr[1]);
  const int HB = TH + 2 * Rr[1], WC = TW + 2 * Rr[0];
  return {std::max(WA * HA, 3 * WC * (HB + 1)), std::max(2 * WA * HB, 3 * HB * (TW + 1))};
}

// 2D: one tensor generation from v->img by the fused kernel.  ev: events around it (ev[0],
// ev[1]; ev[2..5] follow at once so the 3D bookkeeping holds).
template <typename T>
void ced2_generate(mad_ced_ctx* v, int mode, double* D, int64_t cs, double* lam, Event* ev) {
  hipStream_t st = v->mad->stream;
  const int nx = (int)v->n[0], ny = (int)v->n[1];
  const int* Rs = v->Rs;
  const int* Rr = v->Rr;
  auto bytes = [&](int TW, int TH) {
    const Ced2Lds l = ced2_lds(TW, TH, Rs, Rr);
    return ((size_t)l.s1 + l.s2) * sizeof(T);
  };
  // 64 x 32 outputs per block of 256 threads.  Rows are halved first (the x row stays one
  // wave wide): down to 8 while that brings the block under half a CU's 160 KiB of LDS (two
  // blocks per CU hide each other's barriers), then, rows before columns, as far as the taps
  // need to fit at all.  Below 16 x 4 the halo is all of the tile's work.
  int TW = 64, TH = 32;
  while (TH > 8 && bytes(TW, TH) > 80 * 1024) TH /= 2;
  while (TH > 4 && bytes(TW, TH) > kVedLds) TH /= 2;
  while (TW > 16 && bytes(TW, TH) > kVedLds) TW /= 2;
  const size_t lds = bytes(TW, TH);
  REQUIRE(lds <= kVedLds, MAD_ERR_UNSUPPORTED,
          "Gaussian taps too long for the LDS tiles (scale / spacing too large)");
  v->tile[0] = TW;
  v->tile[1] = TH;
  ced2_lds_attr<T>();
  const T* tp = (const T*)v->taps;
  const double* h = v->d.spacing;
  const CedParams cp{v->d.enhancement, v->d.contrast * v->d.contrast, v->d.exponent, v->d.alpha};
  const dim3 grid((nx + TW - 1) / TW, (ny + TH - 1) / TH);
  const int s1 = ced2_lds(TW, TH, Rs, Rr).s1;
  if (ev) HIP_CHECK(hipEventRecord(ev[0], st));
  if (mode == CED_STRUCTURE)
    hipLaunchKernelGGL((ced2_k<T, CED_STRUCTURE>), grid, dim3(256), lds, st, v->img, tp + v->tap_off[0],
                       tp + v->tap_off[1], Rs[0], Rs[1], Rr[0], Rr[1], nx, ny, TW, TH, s1, (T)(1.0 / h[0]),
                       (T)(1.0 / h[1]), cs, D, nullptr, cp);
  else
    hipLaunchKernelGGL((ced2_k<T, CED_TENSOR>), grid, dim3(256), lds, st, v->img, tp + v->tap_off[0],
                       tp + v->tap_off[1], Rs[0], Rs[1], Rr[0], Rr[1], nx, ny, TW, TH, s1, (T)(1.0 / h[0]),
                       (T)(1.0 / h[1]), cs, D, lam, cp);
  if (ev)
    for (int q = 1; q < 6; ++q) HIP_CHECK(hipEventRecord(ev[q], st));
  HIP_CHECK(hipGetLastError());
}

void ced_generate_any(mad_ced_ctx* v, int mode, double* D, int64_t cs, double* lam, Event* ev) {
  const bool f64 = v->d.precision == MAD_FP64;
  if (v->dim == 2 && f64) ced2_generate<double>(v, mode, D, cs, lam, ev);
  else if (v->dim == 2) ced2_generate<float>(v, mode, D, cs, lam, ev);
  else if (f64) ced_generate<double>(v, mode, D, cs, lam, ev);
  else ced_generate<float>(v, mode, D, cs, lam, ev);
}

// the tensor of v->img into the solver's tensor storage; the solver's setup is redone
void ced_tensor_to_solver(mad_ced_ctx* v, double* lam, Event* ev) {
  mad_ctx* c = v->mad;
  tensor_alloc(c);
  ced_generate_any(v, CED_TENSOR, tensor_at0(c), c->tensor_cs, lam, ev);
  c->tensor_set = true;
  c->setup_done = false;
}

void ced_run_impl(mad_ced_ctx* v, const void* in, int in_dt, void* out, int out_dt, bool dev,
                  mad_ced_stats* st) {
  mad_ctx* c = v->mad;
  HIP_CHECK(hipSetDevice(c->device));
  const size_t oes = dtype_size(out_dt);
  REQUIRE(oes, MAD_ERR_INVALID, "bad output dtype");
  ced_load_image(v, in, in_dt, dev);
  Event ev[6], done;
  double pass_ms[5] = {0, 0, 0, 0, 0}, diff_ms = 0.0, relres = 0.0;
  unsigned cycles = 0;
  int stalled = 0;
  for (uint32_t it = 0; it < v->d.iterations; ++it) {
    if (v->d.verbose) std::printf("Iteration n.%u...\n", it + 1);
    ced_tensor_to_solver(v, nullptr, ev);
    mad_stats ms{};
    mad_call(c, run_impl(c, v->img, MAD_F64, v->img2, MAD_F64, &ms, true));
    std::swap(v->img, v->img2);
    HIP_CHECK(hipEventRecord(done, c->stream));
    HIP_CHECK(hipEventSynchronize(done));
    // 2D: the fused kernel is pass 0, the others stay 0
    for (int q = 0; q < (v->dim == 2 ? 1 : 5); ++q) pass_ms[q] += elapsed(ev[q], ev[q + 1]);
    diff_ms += elapsed(ev[5], done);
    cycles += ms.total_cycles;
    relres = ms.last_relres;
    stalled |= ms.stalled;
  }
  void* dst = dev ? out : ced_stage(v, oes * v->N);
  convert_from<double>(v->img, dst, out_dt, v->N, c->stream);
  if (!dev) HIP_CHECK(hipMemcpyAsync(out, dst, oes * v->N, hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->iterations = v->d.iterations;
    st->total_cycles = cycles;
    st->last_relres = relres;
    for (int q = 0; q < 5; ++q) {
      st->pass_ms[q] = pass_ms[q];
      st->tensor_ms += pass_ms[q];
    }
    st->diffusion_ms = diff_ms;
    st->stalled = stalled;
    st->tile[0] = v->tile[0];
    st->tile[1] = v->tile[1];
  }
}

// as mad_ved_run: MAD_ERR_NOT_CONVERGED (output written) when a diffusion step stalled
int ced_run_status(mad_ced_ctx* v, int rc, const mad_ced_stats& st) {
  if (rc != MAD_OK || !st.stalled) return rc;
  char buf[200];
  std::snprintf(buf, sizeof buf,
                "tolerance %g not reached: the stall guard ended a diffusion step at relres %g (the "
                "storage precision's floor)", v->d.tolerance, st.last_relres);
  v->err = buf;
  return MAD_ERR_NOT_CONVERGED;
}

}  // namespace

extern "C" {

int mad_ced_desc_init(mad_ced_desc* d) {
  if (!d) return MAD_ERR_INVALID;
  std::memset(d, 0, sizeof(*d));
  d->abi_version = MAD_ABI_VERSION;
  d->size[0] = d->size[1] = d->size[2] = 1;
  d->spacing[0] = d->spacing[1] = d->spacing[2] = 1.0;
  d->enhancement = MAD_CED_EED;
  d->noise_scale = 0.5;
  d->feature_scale = 2.0;
  d->contrast = 1.0;
  d->exponent = 2.0;
  d->alpha = 0.01;
  d->iterations = 1;
  d->diffusion_iterations = 5;
  d->cycle = MAD_VCYCLE;
  d->time_step = 0.1;
  d->tolerance = 1e-6;
  d->diffusion_iterations_per_grid = 2;
  d->smoother = MAD_GAUSS_SEIDEL;
  d->precision = MAD_PRECISION_AUTO;
  d->device = -1;
  d->dim = 3;
  return MAD_OK;
}

int mad_ced_create(const mad_ced_desc* d, mad_ced_ctx** out) {
  if (!out) return MAD_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<mad_ced_ctx> v(new mad_ced_ctx());
  int rc = ced_guarded(nullptr, [&] {
    REQUIRE(d, MAD_ERR_INVALID, "null descriptor");
    REQUIRE(d->abi_version == MAD_ABI_VERSION, MAD_ERR_INVALID, "ABI version mismatch");
    REQUIRE(d->enhancement == MAD_CED_EED || d->enhancement == MAD_CED_CED, MAD_ERR_INVALID,
            "unknown enhancement (MAD_CED_EED or MAD_CED_CED)");
    REQUIRE(d->noise_scale > 0.0 && d->feature_scale > 0.0, MAD_ERR_INVALID,
            "noise_scale and feature_scale must be positive");
    REQUIRE(d->contrast > 0.0, MAD_ERR_INVALID, "contrast must be positive");
    REQUIRE(d->exponent > 0.0, MAD_ERR_INVALID, "exponent must be positive");
    REQUIRE(d->alpha > 0.0 && d->alpha < 1.0, MAD_ERR_INVALID, "alpha must lie in (0, 1)");
    REQUIRE(d->options == 0, MAD_ERR_INVALID, "unknown option bits");
    // dim 0: a caller built against the header that had no dim there (reserved, zero)
    const int dim = d->dim == 0 ? 3 : d->dim;
    REQUIRE(dim == 2 || dim == 3, MAD_ERR_INVALID, "dim must be 2 or 3 (0 is read as 3)");
    REQUIRE(dim == 3 || d->size[2] == 1, MAD_ERR_INVALID, "dim 2 needs size[2] == 1");
    for (int q = 0; q < dim; ++q)
      REQUIRE(d->spacing[q] > 0.0, MAD_ERR_INVALID, "spacing must be positive");
    v->d = *d;
    v->dim = dim;
    mad_desc md;
    mad_desc_init(&md);
    md.dim = dim;
    for (int q = 0; q < 3; ++q) {
      md.size[q] = d->size[q];
      md.spacing[q] = q < dim ? d->spacing[q] : 1.0;
    }
    md.cycle = d->cycle;
    md.smoother = d->smoother;
    md.iterations_per_grid = d->diffusion_iterations_per_grid;
    md.max_cycles = 100;
    md.number_of_steps = d->diffusion_iterations;
    md.time_step = d->time_step;
    md.tolerance = d->tolerance;
    md.verbose = d->verbose;
    md.precision = d->precision;
    md.device = d->device;
    // the tensor is new in every iteration, so setup is redone each time: the placement
    // tuner's trial allocations would be paid per iteration
    md.options = MAD_OPT_NO_PLACEMENT_TUNE;
    const int mrc = mad_create(&md, &v->mad);
    if (mrc != MAD_OK) throw MadError(mrc, g_last_error);
    for (int q = 0; q < 3; ++q) v->n[q] = d->size[q];
    v->N = v->n[0] * v->n[1] * v->n[2];
    REQUIRE(v->n[0] <= INT32_MAX - 1024 && v->n[1] <= 65535 && v->n[2] <= 65535, MAD_ERR_INVALID,
            "image too large for the structure-tensor grid mapping");
    HIP_CHECK(hipSetDevice(v->mad->device));
    HIP_CHECK(big_alloc((void**)&v->img, sizeof(double) * v->N));
    HIP_CHECK(big_alloc((void**)&v->img2, sizeof(double) * v->N));
    if (d->precision == MAD_FP64) ced_upload_taps<double>(v.get());
    else ced_upload_taps<float>(v.get());
  });
  if (rc != MAD_OK) return rc;
  *out = v.release();
  return MAD_OK;
}

void mad_ced_destroy(mad_ced_ctx* v) { delete v; }

const char* mad_ced_last_error(const mad_ced_ctx* v) { return v ? v->err.c_str() : g_last_error.c_str(); }

int mad_ced_run(mad_ced_ctx* v, const void* in, int32_t in_dtype, void* out, int32_t out_dtype,
                mad_ced_stats* st) {
  if (!v || !in || !out) return MAD_ERR_INVALID;
  mad_ced_stats local{};
  mad_ced_stats* s = st ? st : &local;
  return ced_run_status(v, ced_guarded(v, [&] { ced_run_impl(v, in, in_dtype, out, out_dtype, false, s); }), *s);
}

int mad_ced_run_device(mad_ced_ctx* v, const void* in, int32_t in_dtype, void* out, int32_t out_dtype,
                       mad_ced_stats* st) {
  if (!v || !in || !out) return MAD_ERR_INVALID;
  mad_ced_stats local{};
  mad_ced_stats* s = st ? st : &local;
  return ced_run_status(v, ced_guarded(v, [&] { ced_run_impl(v, in, in_dtype, out, out_dtype, true, s); }), *s);
}

int mad_ced_tensor(mad_ced_ctx* v, const void* image, int32_t dtype, double* tensor_soa, double* lambda_soa) {
  if (!v || !image || !tensor_soa) return MAD_ERR_INVALID;
  return ced_guarded(v, [&] {
    HIP_CHECK(hipSetDevice(v->mad->device));
    ced_load_image(v, image, dtype, false);
    const int nc = v->dim == 2 ? 3 : 6;  // tensor components; dim mapped eigenvalues
    if (lambda_soa && !v->lam) HIP_CHECK(big_alloc((void**)&v->lam, sizeof(double) * v->dim * v->N));
    ced_tensor_to_solver(v, lambda_soa ? v->lam : nullptr, nullptr);
    hipStream_t st = v->mad->stream;
    // one rank: the solver's tensor is the whole grid, component stride N
    HIP_CHECK(hipMemcpyAsync(tensor_soa, tensor_at0(v->mad), sizeof(double) * nc * v->N, hipMemcpyDeviceToHost, st));
    if (lambda_soa)
      HIP_CHECK(hipMemcpyAsync(lambda_soa, v->lam, sizeof(double) * v->dim * v->N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int mad_ced_structure_tensor(mad_ced_ctx* v, const void* image, int32_t dtype, double* structure_soa) {
  if (!v || !image || !structure_soa) return MAD_ERR_INVALID;
  return ced_guarded(v, [&] {
    HIP_CHECK(hipSetDevice(v->mad->device));
    ced_load_image(v, image, dtype, false);
    const int nc = v->dim == 2 ? 3 : 6;
    double* J = nullptr;
    HIP_CHECK(big_alloc((void**)&J, sizeof(double) * nc * v->N));
    std::unique_ptr<double, void (*)(double*)> hold(J, [](double* p) { (void)hipFree(p); });
    ced_generate_any(v, CED_STRUCTURE, J, v->N, nullptr, nullptr);
    HIP_CHECK(hipMemcpyAsync(structure_soa, J, sizeof(double) * nc * v->N, hipMemcpyDeviceToHost,
                             v->mad->stream));
    HIP_CHECK(hipStreamSynchronize(v->mad->stream));
  });
}

}  // extern "C"
