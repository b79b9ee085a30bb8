// mad_pm.hpp -- host driver + C ABI of include/mad_pm.h (regularised Perona-Malik diffusion on
// the GPU).  Included at the end of mad_solver.hip, after mad_ced.hpp, whose helpers it shares
// (ced_guarded, ced_lds_attr and the z / y gradient passes): like the CED driver it hands the
// device tensor to the MAD solver in place (tensor_at0) and runs the diffusion steps through
// run_impl, no host round trips between tensor generation and solve.
#include "../../include/mad_pm.h"
#include "../../include/mad_pm_quantile.h"
#include "mad_pm_kernels.hpp"
#include "mad_select.hpp"

struct mad_pm_ctx {
  mad_pm_desc d{};
  std::string err;
  mad_ctx* mad = nullptr;  // the diffusion solver, kept across iterations
  int dim = 3;             // 2: the fused kernel pm2_k, tensor [xx,xy,yy]
  int tile[2] = {0, 0};    // 2D: the output tile of the last tensor generation (x, y)
  int64_t n[3] = {0, 0, 0};
  int64_t N = 0;
  int C = 1;               // channels (mad_pm_desc.channels, 0 read as 1); images are C planes of N
  double* img = nullptr;   // internal image (fp64), C N
  double* img2 = nullptr;  // next iterate, C N
  void* vol = nullptr;     // 3D: 3 C + 2 scratch volumes in the storage precision (C = 1: the 5 of
                           // the scalar passes)
  void* taps = nullptr;    // device taps, per axis [K0 | K1 | 0 0 0 K0 0 0 0 | 0 0 0 K1 0 0 0]
  int R[3] = {0, 0, 0};
  size_t tap_off[3] = {0, 0, 0};  // element offset of each axis' taps
  double* gdev = nullptr;  // the diffusivity (mad_pm_tensor only)
  void* stage = nullptr;   // host <-> device staging
  size_t stage_bytes = 0;
  // quantile mode, mad_pm_contrast and mad_pm_select only; all allocated on first use
  bool quantile = false;   // contrast_mode == MAD_PM_CONTRAST_QUANTILE
  void* sq = nullptr;      // s in the storage precision
  SelScratch sel;          // the selection's histograms, state and candidate list
  // pinned, two words, each copied behind its selection on the stream: [kK2Generation] K^2 of the
  // last tensor generation, [kK2Inspection] the result of mad_pm_contrast / mad_pm_select
  double* k2_host = nullptr;
  ~mad_pm_ctx() {
    if (mad) (void)hipSetDevice(mad->device);
    if (mad && mad->stream) (void)hipStreamSynchronize(mad->stream);
    for (void* p : {(void*)img, (void*)img2, vol, taps, (void*)gdev, stage, sq, sel.work, sel.list})
      if (p) (void)hipFree(p);
    if (k2_host) (void)hipHostFree(k2_host);
    if (mad) mad_destroy(mad);
  }
};

namespace {

enum { kK2Generation = 0, kK2Inspection = 1 };

// ced_guarded's status mapping, the message kept on this context
template <typename F>
int pm_guarded(mad_pm_ctx* v, F&& f) {
  const int rc = ced_guarded(nullptr, f);
  if (rc != MAD_OK && v) v->err = g_last_error;
  return rc;
}

void* pm_stage(mad_pm_ctx* v, size_t bytes) {
  if (bytes > v->stage_bytes) {
    if (v->stage) HIP_CHECK(hipFree(v->stage));
    v->stage = nullptr;
    v->stage_bytes = 0;
    HIP_CHECK(hipMalloc(&v->stage, bytes));
    v->stage_bytes = bytes;
  }
  return v->stage;
}

// host or device image (any dtype, all C planes) -> v->img (fp64)
void pm_load_image(mad_pm_ctx* v, const void* src, int dt, bool dev) {
  const size_t es = dtype_size(dt);
  REQUIRE(es, MAD_ERR_INVALID, "bad image dtype");
  hipStream_t st = v->mad->stream;
  const int64_t n = v->C * v->N;
  if (!dev) {
    void* s = pm_stage(v, es * n);
    HIP_CHECK(hipMemcpyAsync(s, src, es * n, hipMemcpyHostToDevice, st));
    src = s;
  }
  convert_to<double>(src, dt, v->img, n, st);
}

// allow the new kernels more than the default 64 KiB of dynamic LDS (once per type)
template <typename T>
void pm_lds_attr() {
  static bool done = false;
  if (done) return;
  for (const void* k : {(const void*)pm_x_k<T, PM_TENSOR>, (const void*)pm_x_k<T, PM_GRADIENT>,
                        (const void*)pm_x_k<T, PM_SQNORM>, (const void*)pm2_k<T, PM_TENSOR>,
                        (const void*)pm2_k<T, PM_GRADIENT>, (const void*)pm2_k<T, PM_SQNORM>,
                        (const void*)pmv_x_k<T, PM_TENSOR>, (const void*)pmv_x_k<T, PM_GRADIENT>,
                        (const void*)pmv_x_k<T, PM_SQNORM>, (const void*)pm2v_k<T, PM_TENSOR>,
                        (const void*)pm2v_k<T, PM_GRADIENT>, (const void*)pm2v_k<T, PM_SQNORM>})
    HIP_CHECK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVedLds));
  done = true;
}

// the sigma taps on every axis (ved_taps: the VED FIR operator's K0, K1), in the storage
// precision, uploaded once.  After the plain [K0 | K1] each axis carries both again with three
// zeros on either side, for pm2_k's four-outputs-per-thread x phase.
template <typename T>
void pm_upload_taps(mad_pm_ctx* v) {
  std::vector<T> kt;
  for (int q = 0; q < v->dim; ++q) {
    std::vector<double> K;
    v->R[q] = ved_taps(v->d.noise_scale, v->d.spacing[q], K);
    const int W = 2 * v->R[q] + 1;
    v->tap_off[q] = kt.size();
    for (int t = 0; t < 2 * W; ++t) kt.push_back((T)K[t]);  // K0 | K1
    for (int o = 0; o < 2; ++o) {
      kt.insert(kt.end(), 3, T(0));
      for (int t = 0; t < W; ++t) kt.push_back((T)K[o * W + t]);
      kt.insert(kt.end(), 3, T(0));
    }
  }
  HIP_CHECK(hipMalloc(&v->taps, sizeof(T) * kt.size()));
  HIP_CHECK(hipMemcpy(v->taps, kt.data(), sizeof(T) * kt.size(), hipMemcpyHostToDevice));
}

// the map's parameters in absolute mode (quantile mode: k2 comes from the selection)
PmParams pm_params(const mad_pm_ctx* v) {
  const bool squared = v->d.options & MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED;
  return {v->d.diffusivity, squared ? v->d.contrast : v->d.contrast * v->d.contrast, v->d.exponent, v->d.alpha};
}

// the rank of the quantile q among n values (include/mad_pm.h): numpy's inverted_cdf
int64_t pm_rank(double q, int64_t n) {
  const int64_t k = (int64_t)std::ceil(q * (double)n) - 1;
  return std::min<int64_t>(n - 1, std::max<int64_t>(0, k));
}

// the selection's scratch for n keys of key_bytes, on first use (the list grows on demand)
void pm_select_scratch(mad_pm_ctx* v, int64_t n, size_t key_bytes) {
  REQUIRE(n < ((int64_t)1 << 32), MAD_ERR_UNSUPPORTED, "the selection counts in 32 bits: fewer than 2^32 values");
  if (!v->sel.work) HIP_CHECK(hipMalloc(&v->sel.work, SelScratch::work_bytes));
  if (!v->k2_host) HIP_CHECK(hipHostMalloc((void**)&v->k2_host, 2 * sizeof(double), hipHostMallocDefault));
  const size_t need = n >= kSelListMin ? key_bytes * (size_t)n : 0;
  if (need > v->sel.list_bytes) {
    if (v->sel.list) HIP_CHECK(hipFree(v->sel.list));
    v->sel.list = nullptr;
    v->sel.list_bytes = 0;
    HIP_CHECK(big_alloc(&v->sel.list, need));
    v->sel.list_bytes = need;
  }
}

// Quantile mode behind a PM_SQNORM pass: selects s_q among v->sq (rank of q), leaves K^2 in device
// memory and sends a copy to v->k2_host behind it (with D, a tensor generation: the generation's
// word, else the inspection's); with D, maps s -> g -> D.  No host
// synchronisation: the phases follow each other on the stream.
template <typename T>
void pm_select_and_map(mad_pm_ctx* v, double q, double* D, int64_t cs, double* gout) {
  using Key = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
  hipStream_t st = v->mad->stream;
  HIP_CHECK(select_launch<Key>(v->sel, (const Key*)v->sq, v->N, pm_rank(q, v->N), st));
  HIP_CHECK(hipMemcpyAsync(v->k2_host + (D ? kK2Generation : kK2Inspection), v->sel.value(), sizeof(double),
                           hipMemcpyDeviceToHost, st));
  if (!D) return;
  const unsigned blocks = (unsigned)std::min<int64_t>((v->N + 255) / 256, 8192);
  const PmParams pp = pm_params(v);
  if (v->dim == 2)
    hipLaunchKernelGGL((pm_map_k<T, 3>), dim3(blocks), dim3(256), 0, st, (const T*)v->sq, v->sel.value(), v->N, cs,
                       D, gout, pp);
  else
    hipLaunchKernelGGL((pm_map_k<T, 6>), dim3(blocks), dim3(256), 0, st, (const T*)v->sq, v->sel.value(), v->N, cs,
                       D, gout, pp);
}

// s of v->img in the storage precision, on first use
template <typename T>
T* pm_sq(mad_pm_ctx* v) {
  pm_select_scratch(v, v->N, sizeof(T));
  if (!v->sq) HIP_CHECK(big_alloc(&v->sq, sizeof(T) * v->N));
  return (T*)v->sq;
}

// One 3D tensor generation from v->img: ced_z_k, ced_y_k, pm_x_k.  mode PM_TENSOR: D = the
// tensor (component stride cs), gout optional; PM_GRADIENT: D = (gx, gy, gz).  ev: four events
// around the passes (may be null).  q > 0 (quantile mode): the x pass stores s alone, then the
// selection of the quantile q and, in PM_TENSOR, the map kernel follow (PM_SQNORM: K^2 only, D
// unused); all three count with the last pass.
template <typename T>
void pm_generate(mad_pm_ctx* v, int mode, double* D, int64_t cs, double* gout, Event* ev, double q) {
  hipStream_t st = v->mad->stream;
  const int nx = (int)v->n[0], ny = (int)v->n[1], nz = (int)v->n[2];
  const int64_t N = v->N;
  const int* R = v->R;
  // tiles: z / y tiles shrink with long taps (as ced_generate's); the x row is 256 wide
  auto lds_for = [](int lines, int width, int copies) { return (size_t)lines * width * copies * sizeof(T); };
  int ZT = 32, YT = 32;
  while (ZT > 4 && lds_for(ZT + 2 * R[2], 256, 1) > kVedLds) ZT /= 2;
  while (YT > 4 && lds_for(YT + 2 * R[1], 64, 2) > kVedLds) YT /= 2;
  const size_t l1 = lds_for(ZT + 2 * R[2], 256, 1), l2 = lds_for(YT + 2 * R[1], 64, 2);
  const size_t l3 = lds_for(256 + 2 * R[0], 1, 3);
  REQUIRE(l1 <= kVedLds && l2 <= kVedLds && l3 <= kVedLds, MAD_ERR_UNSUPPORTED,
          "Gaussian taps too long for the LDS tiles (scale / spacing too large)");
  const int C = v->C;
  if (!v->vol) HIP_CHECK(big_alloc((void**)&v->vol, sizeof(T) * (3 * C + 2) * N));
  T* sq = q > 0.0 ? pm_sq<T>(v) : nullptr;
  T* f = (T*)v->vol;
  T *z0 = f, *z1 = f + N, *a00 = f + 2 * N, *a10 = f + 3 * N, *a01 = f + 4 * N;
  ced_lds_attr<T>();
  pm_lds_attr<T>();
  const T* tp = (const T*)v->taps;
  const double* h = v->d.spacing;
  const T ihx = (T)(1.0 / h[0]), ihy = (T)(1.0 / h[1]), ihz = (T)(1.0 / h[2]);
  const PmParams pp = pm_params(v);
  if (ev) HIP_CHECK(hipEventRecord(ev[0], st));
  if (C > 1) {
    // vector-valued: z and y passes per channel through the one pair z0, z1 into the channel's
    // three pass-2 volumes, then the joint x pass.  ev[1] follows the first channel's z pass:
    // pass_ms[1] holds every pass between it and the x pass.
    for (int ch = 0; ch < C; ++ch) {
      T* a = a00 + (int64_t)(3 * ch) * N;
      hipLaunchKernelGGL((ced_z_k<T>), dim3((nx + 63) / 64, (ny + 3) / 4, (nz + ZT - 1) / ZT), dim3(256), l1, st,
                         v->img + (int64_t)ch * N, z0, z1, tp + v->tap_off[2], R[2], nx, ny, nz, ZT);
      if (ev && ch == 0) HIP_CHECK(hipEventRecord(ev[1], st));
      hipLaunchKernelGGL((ced_y_k<T>), dim3((nx + 63) / 64, (ny + YT - 1) / YT, nz), dim3(256), l2, st, z0, z1,
                         a, a + N, a + 2 * N, tp + v->tap_off[1], R[1], nx, ny, nz, YT);
    }
    if (ev) HIP_CHECK(hipEventRecord(ev[2], st));
    const dim3 g3((nx + 255) / 256, ny, nz);
    if (mode == PM_GRADIENT) {
      hipLaunchKernelGGL((pmv_x_k<T, PM_GRADIENT>), g3, dim3(256), l3, st, a00, C, N, tp + v->tap_off[0], R[0], nx,
                         ny, nz, ihx, ihy, ihz, cs, D, nullptr, pp);
    } else if (sq) {
      hipLaunchKernelGGL((pmv_x_k<T, PM_SQNORM>), g3, dim3(256), l3, st, a00, C, N, tp + v->tap_off[0], R[0], nx,
                         ny, nz, ihx, ihy, ihz, cs, (double*)sq, nullptr, pp);
      pm_select_and_map<T>(v, q, mode == PM_TENSOR ? D : nullptr, cs, gout);
    } else
      hipLaunchKernelGGL((pmv_x_k<T, PM_TENSOR>), g3, dim3(256), l3, st, a00, C, N, tp + v->tap_off[0], R[0], nx,
                         ny, nz, ihx, ihy, ihz, cs, D, gout, pp);
    if (ev) HIP_CHECK(hipEventRecord(ev[3], st));
    HIP_CHECK(hipGetLastError());
    return;
  }
  hipLaunchKernelGGL((ced_z_k<T>), dim3((nx + 63) / 64, (ny + 3) / 4, (nz + ZT - 1) / ZT), dim3(256), l1, st,
                     v->img, z0, z1, tp + v->tap_off[2], R[2], nx, ny, nz, ZT);
  if (ev) HIP_CHECK(hipEventRecord(ev[1], st));
  hipLaunchKernelGGL((ced_y_k<T>), dim3((nx + 63) / 64, (ny + YT - 1) / YT, nz), dim3(256), l2, st, z0, z1,
                     a00, a10, a01, tp + v->tap_off[1], R[1], nx, ny, nz, YT);
  if (ev) HIP_CHECK(hipEventRecord(ev[2], st));
  const dim3 g3((nx + 255) / 256, ny, nz);
  if (mode == PM_GRADIENT) {
    hipLaunchKernelGGL((pm_x_k<T, PM_GRADIENT>), g3, dim3(256), l3, st, a00, a10, a01, tp + v->tap_off[0],
                       R[0], nx, ny, nz, ihx, ihy, ihz, cs, D, nullptr, pp);
  } else if (sq) {
    hipLaunchKernelGGL((pm_x_k<T, PM_SQNORM>), g3, dim3(256), l3, st, a00, a10, a01, tp + v->tap_off[0], R[0],
                       nx, ny, nz, ihx, ihy, ihz, cs, (double*)sq, nullptr, pp);
    pm_select_and_map<T>(v, q, mode == PM_TENSOR ? D : nullptr, cs, gout);
  } else
    hipLaunchKernelGGL((pm_x_k<T, PM_TENSOR>), g3, dim3(256), l3, st, a00, a10, a01, tp + v->tap_off[0], R[0],
                       nx, ny, nz, ihx, ihy, ihz, cs, D, gout, pp);
  if (ev) HIP_CHECK(hipEventRecord(ev[3], st));
  HIP_CHECK(hipGetLastError());
}

// The LDS regions of pm2_k for a TW x TH tile, in elements: R1 = image tile | gx, gy (row pitch
// TW + 1), R2 = K0y u, K1y u (column-major, pitch TH + 1); the kernel's comment names the phases.
struct Pm2Lds {
  int s1, s2;
};
Pm2Lds pm2_lds(int TW, int TH, const int* R) {
  const int WA = TW + 2 * R[0], HA = TH + 2 * R[1];
  return {std::max(WA * HA, 2 * TH * (TW + 1)), 2 * WA * (TH + 1)};
}

// 2D: one tensor generation from v->img by the fused kernel.  ev: events around it (ev[0],
// ev[1]; ev[2..3] follow at once so the 3D bookkeeping holds).  q as in pm_generate.
template <typename T>
void pm2_generate(mad_pm_ctx* v, int mode, double* D, int64_t cs, double* gout, Event* ev, double q) {
  hipStream_t st = v->mad->stream;
  const int nx = (int)v->n[0], ny = (int)v->n[1];
  const int* R = v->R;
  auto bytes = [&](int TW, int TH) {
    const Pm2Lds l = pm2_lds(TW, TH, R);
    return ((size_t)l.s1 + l.s2) * sizeof(T);
  };
  // 64 x 32 outputs per block of 256 threads, the plan of ced2_generate.  Rows are halved
  // first (the x row stays one wave wide): down to 8 while that brings the block under half a
  // CU's 160 KiB of LDS (two blocks per CU hide each other's barriers), then, rows before
  // columns, as far as the taps need to fit at all.  Below 16 x 4 the halo is all of the
  // tile's work.
  int TW = 64, TH = 32;
  while (TH > 8 && bytes(TW, TH) > 80 * 1024) TH /= 2;
  while (TH > 4 && bytes(TW, TH) > kVedLds) TH /= 2;
  while (TW > 16 && bytes(TW, TH) > kVedLds) TW /= 2;
  const size_t lds = bytes(TW, TH);
  REQUIRE(lds <= kVedLds, MAD_ERR_UNSUPPORTED,
          "Gaussian taps too long for the LDS tiles (scale / spacing too large)");
  v->tile[0] = TW;
  v->tile[1] = TH;
  T* sq = q > 0.0 ? pm_sq<T>(v) : nullptr;
  pm_lds_attr<T>();
  const T* tp = (const T*)v->taps;
  const T* txp = tp + v->tap_off[0] + 2 * (2 * R[0] + 1);  // the padded x taps
  const T* ty = tp + v->tap_off[1];
  const double* h = v->d.spacing;
  const T ihx = (T)(1.0 / h[0]), ihy = (T)(1.0 / h[1]);
  const PmParams pp = pm_params(v);
  const dim3 grid((nx + TW - 1) / TW, (ny + TH - 1) / TH);
  const int s1 = pm2_lds(TW, TH, R).s1;
  if (ev) HIP_CHECK(hipEventRecord(ev[0], st));
  const int C = v->C;
  if (C > 1) {
    // vector-valued: the channel loop runs inside the kernel, on the same tile and LDS
    if (mode == PM_GRADIENT) {
      hipLaunchKernelGGL((pm2v_k<T, PM_GRADIENT>), grid, dim3(256), lds, st, v->img, C, v->N, txp, ty, R[0], R[1],
                         nx, ny, TW, TH, s1, ihx, ihy, cs, D, nullptr, pp);
    } else if (sq) {
      hipLaunchKernelGGL((pm2v_k<T, PM_SQNORM>), grid, dim3(256), lds, st, v->img, C, v->N, txp, ty, R[0], R[1], nx,
                         ny, TW, TH, s1, ihx, ihy, cs, (double*)sq, nullptr, pp);
      pm_select_and_map<T>(v, q, mode == PM_TENSOR ? D : nullptr, cs, gout);
    } else
      hipLaunchKernelGGL((pm2v_k<T, PM_TENSOR>), grid, dim3(256), lds, st, v->img, C, v->N, txp, ty, R[0], R[1], nx,
                         ny, TW, TH, s1, ihx, ihy, cs, D, gout, pp);
  } else if (mode == PM_GRADIENT) {
    hipLaunchKernelGGL((pm2_k<T, PM_GRADIENT>), grid, dim3(256), lds, st, v->img, txp, ty, R[0], R[1], nx, ny,
                       TW, TH, s1, ihx, ihy, cs, D, nullptr, pp);
  } else if (sq) {
    hipLaunchKernelGGL((pm2_k<T, PM_SQNORM>), grid, dim3(256), lds, st, v->img, txp, ty, R[0], R[1], nx, ny, TW,
                       TH, s1, ihx, ihy, cs, (double*)sq, nullptr, pp);
    pm_select_and_map<T>(v, q, mode == PM_TENSOR ? D : nullptr, cs, gout);
  } else
    hipLaunchKernelGGL((pm2_k<T, PM_TENSOR>), grid, dim3(256), lds, st, v->img, txp, ty, R[0], R[1], nx, ny, TW,
                       TH, s1, ihx, ihy, cs, D, gout, pp);
  if (ev)
    for (int q = 1; q < 4; ++q) HIP_CHECK(hipEventRecord(ev[q], st));
  HIP_CHECK(hipGetLastError());
}

// q: the quantile of quantile mode (PM_TENSOR in a quantile context, PM_SQNORM anywhere), else 0
void pm_generate_any(mad_pm_ctx* v, int mode, double* D, int64_t cs, double* gout, Event* ev, double q = 0.0) {
  const bool f64 = v->d.precision == MAD_FP64;
  if (v->dim == 2 && f64) pm2_generate<double>(v, mode, D, cs, gout, ev, q);
  else if (v->dim == 2) pm2_generate<float>(v, mode, D, cs, gout, ev, q);
  else if (f64) pm_generate<double>(v, mode, D, cs, gout, ev, q);
  else pm_generate<float>(v, mode, D, cs, gout, ev, q);
}

// K of a run's last tensor generation (generated: the run had one); quantile mode: valid once the
// stream has been synchronised, and 0 for a run without a generation (iterations = 0)
double pm_contrast_used(const mad_pm_ctx* v, bool generated) {
  if (v->quantile) return generated && v->k2_host ? std::sqrt(v->k2_host[kK2Generation]) : 0.0;
  return v->d.options & MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED ? std::sqrt(v->d.contrast) : v->d.contrast;
}

// the tensor of v->img into the solver's tensor storage; the solver's setup is redone
void pm_tensor_to_solver(mad_pm_ctx* v, double* gout, Event* ev) {
  mad_ctx* c = v->mad;
  tensor_alloc(c);
  pm_generate_any(v, PM_TENSOR, tensor_at0(c), c->tensor_cs, gout, ev, v->quantile ? v->d.contrast : 0.0);
  c->tensor_set = true;
  c->setup_done = false;
}

void pm_run_impl(mad_pm_ctx* v, const void* in, int in_dt, void* out, int out_dt, bool dev,
                 mad_pm_stats* st) {
  mad_ctx* c = v->mad;
  HIP_CHECK(hipSetDevice(c->device));
  const size_t oes = dtype_size(out_dt);
  REQUIRE(oes, MAD_ERR_INVALID, "bad output dtype");
  pm_load_image(v, in, in_dt, dev);
  Event ev[4], done;
  double pass_ms[3] = {0, 0, 0}, diff_ms = 0.0, relres = 0.0;
  unsigned cycles = 0;
  int stalled = 0;
  for (uint32_t it = 0; it < v->d.iterations; ++it) {
    if (v->d.verbose) std::printf("Iteration n.%u...\n", it + 1);
    pm_tensor_to_solver(v, nullptr, ev);
    // every channel through the same operators: the first run_impl does the setup
    // (pm_tensor_to_solver cleared setup_done), the others find it done
    mad_stats ms{};
    for (int ch = 0; ch < v->C; ++ch) {
      mad_stats cs{};
      mad_call(c, run_impl(c, v->img + (int64_t)ch * v->N, MAD_F64, v->img2 + (int64_t)ch * v->N, MAD_F64, &cs, true));
      ms.total_cycles += cs.total_cycles;
      ms.last_relres = ch ? std::max(ms.last_relres, cs.last_relres) : cs.last_relres;
      ms.stalled |= cs.stalled;
    }
    std::swap(v->img, v->img2);
    HIP_CHECK(hipEventRecord(done, c->stream));
    HIP_CHECK(hipEventSynchronize(done));
    // 2D: the fused kernel is pass 0, the others stay 0
    for (int q = 0; q < (v->dim == 2 ? 1 : 3); ++q) pass_ms[q] += elapsed(ev[q], ev[q + 1]);
    diff_ms += elapsed(ev[3], done);
    cycles += ms.total_cycles;
    relres = ms.last_relres;
    stalled |= ms.stalled;
  }
  const int64_t cn = v->C * v->N;
  void* dst = dev ? out : pm_stage(v, oes * cn);
  convert_from<double>(v->img, dst, out_dt, cn, c->stream);
  if (!dev) HIP_CHECK(hipMemcpyAsync(out, dst, oes * cn, hipMemcpyDeviceToHost, c->stream));
  HIP_CHECK(hipStreamSynchronize(c->stream));
  if (st) {
    std::memset(st, 0, sizeof(*st));
    st->iterations = v->d.iterations;
    st->total_cycles = cycles;
    st->last_relres = relres;
    for (int q = 0; q < 3; ++q) {
      st->pass_ms[q] = pass_ms[q];
      st->tensor_ms += pass_ms[q];
    }
    st->diffusion_ms = diff_ms;
    st->stalled = stalled;
    st->tile[0] = v->tile[0];
    st->tile[1] = v->tile[1];
    st->contrast_used = pm_contrast_used(v, v->d.iterations > 0);
  }
}

// as mad_ced_run: MAD_ERR_NOT_CONVERGED (output written) when a diffusion step stalled
int pm_run_status(mad_pm_ctx* v, int rc, const mad_pm_stats& st) {
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

int mad_pm_desc_init(mad_pm_desc* d) {
  if (!d) return MAD_ERR_INVALID;
  std::memset(d, 0, sizeof(*d));
  d->abi_version = MAD_ABI_VERSION;
  d->size[0] = d->size[1] = d->size[2] = 1;
  d->spacing[0] = d->spacing[1] = d->spacing[2] = 1.0;
  d->diffusivity = MAD_PM_WEICKERT;
  d->noise_scale = 0.5;
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

int mad_pm_create(const mad_pm_desc* d, mad_pm_ctx** out) {
  if (!out) return MAD_ERR_INVALID;
  *out = nullptr;
  std::unique_ptr<mad_pm_ctx> v(new mad_pm_ctx());
  int rc = pm_guarded(nullptr, [&] {
    REQUIRE(d, MAD_ERR_INVALID, "null descriptor");
    REQUIRE(d->abi_version == MAD_ABI_VERSION, MAD_ERR_INVALID, "ABI version mismatch");
    REQUIRE(d->diffusivity == MAD_PM_WEICKERT || d->diffusivity == MAD_PM_EXPONENTIAL ||
                d->diffusivity == MAD_PM_RATIONAL,
            MAD_ERR_INVALID, "unknown diffusivity (MAD_PM_WEICKERT, MAD_PM_EXPONENTIAL or MAD_PM_RATIONAL)");
    REQUIRE(d->noise_scale > 0.0, MAD_ERR_INVALID, "noise_scale must be positive");
    REQUIRE(d->contrast_mode == MAD_PM_CONTRAST_ABSOLUTE || d->contrast_mode == MAD_PM_CONTRAST_QUANTILE,
            MAD_ERR_INVALID, "unknown contrast_mode (MAD_PM_CONTRAST_ABSOLUTE or MAD_PM_CONTRAST_QUANTILE)");
    REQUIRE(d->channels >= 0 && d->channels <= 16, MAD_ERR_INVALID,
            "channels must lie in 1..16 (0 is read as 1)");
    const bool quantile = d->contrast_mode == MAD_PM_CONTRAST_QUANTILE;
    if (quantile)
      REQUIRE(d->contrast > 0.0 && d->contrast <= 1.0, MAD_ERR_INVALID,
              "MAD_PM_CONTRAST_QUANTILE: contrast holds the quantile q, 0 < q <= 1");
    REQUIRE(d->contrast > 0.0, MAD_ERR_INVALID, "contrast must be positive");
    REQUIRE(d->exponent > 0.0, MAD_ERR_INVALID, "exponent must be positive");
    REQUIRE(d->alpha > 0.0 && d->alpha < 1.0, MAD_ERR_INVALID, "alpha must lie in (0, 1)");
    REQUIRE((d->options & ~MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED) == 0, MAD_ERR_INVALID, "unknown option bits");
    REQUIRE(!(d->options & MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED) || !quantile, MAD_ERR_INVALID,
            "MAD_PM_OPT_TEST_CONTRAST_IS_SQUARED goes with MAD_PM_CONTRAST_ABSOLUTE");
    const int dim = d->dim == 0 ? 3 : d->dim;
    REQUIRE(dim == 2 || dim == 3, MAD_ERR_INVALID, "dim must be 2 or 3 (0 is read as 3)");
    REQUIRE(dim == 3 || d->size[2] == 1, MAD_ERR_INVALID, "dim 2 needs size[2] == 1");
    for (int q = 0; q < dim; ++q)
      REQUIRE(d->spacing[q] > 0.0, MAD_ERR_INVALID, "spacing must be positive");
    if (quantile) {
      // the selection counts in 32 bits
      bool fits = true;
      int64_t total = 1;
      for (int q = 0; q < 3 && fits; ++q) {
        const int64_t nq = d->size[q];
        fits = nq >= 1 && nq <= (int64_t)UINT32_MAX / total;
        if (fits) total *= nq;
      }
      REQUIRE(fits, MAD_ERR_INVALID, "MAD_PM_CONTRAST_QUANTILE needs 1 <= N < 2^32 voxels");
    }
    v->d = *d;
    v->dim = dim;
    v->quantile = quantile;
    v->C = d->channels == 0 ? 1 : d->channels;
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
            "image too large for the gradient passes' grid mapping");
    HIP_CHECK(hipSetDevice(v->mad->device));
    HIP_CHECK(big_alloc((void**)&v->img, sizeof(double) * v->C * v->N));
    HIP_CHECK(big_alloc((void**)&v->img2, sizeof(double) * v->C * v->N));
    if (d->precision == MAD_FP64) pm_upload_taps<double>(v.get());
    else pm_upload_taps<float>(v.get());
  });
  if (rc != MAD_OK) return rc;
  *out = v.release();
  return MAD_OK;
}

void mad_pm_destroy(mad_pm_ctx* v) { delete v; }

const char* mad_pm_last_error(const mad_pm_ctx* v) { return v ? v->err.c_str() : g_last_error.c_str(); }

int mad_pm_run(mad_pm_ctx* v, const void* in, int32_t in_dtype, void* out, int32_t out_dtype,
               mad_pm_stats* st) {
  if (!v || !in || !out) return MAD_ERR_INVALID;
  mad_pm_stats local{};
  mad_pm_stats* s = st ? st : &local;
  return pm_run_status(v, pm_guarded(v, [&] { pm_run_impl(v, in, in_dtype, out, out_dtype, false, s); }), *s);
}

int mad_pm_run_device(mad_pm_ctx* v, const void* in, int32_t in_dtype, void* out, int32_t out_dtype,
                      mad_pm_stats* st) {
  if (!v || !in || !out) return MAD_ERR_INVALID;
  mad_pm_stats local{};
  mad_pm_stats* s = st ? st : &local;
  return pm_run_status(v, pm_guarded(v, [&] { pm_run_impl(v, in, in_dtype, out, out_dtype, true, s); }), *s);
}

int mad_pm_tensor(mad_pm_ctx* v, const void* image, int32_t dtype, double* tensor_soa, double* diffusivity) {
  if (!v || !image || !tensor_soa) return MAD_ERR_INVALID;
  return pm_guarded(v, [&] {
    HIP_CHECK(hipSetDevice(v->mad->device));
    pm_load_image(v, image, dtype, false);
    const int nc = v->dim == 2 ? 3 : 6;
    if (diffusivity && !v->gdev) HIP_CHECK(big_alloc((void**)&v->gdev, sizeof(double) * v->N));
    pm_tensor_to_solver(v, diffusivity ? v->gdev : nullptr, nullptr);
    hipStream_t st = v->mad->stream;
    // one rank: the solver's tensor is the whole grid, component stride N
    HIP_CHECK(hipMemcpyAsync(tensor_soa, tensor_at0(v->mad), sizeof(double) * nc * v->N, hipMemcpyDeviceToHost, st));
    if (diffusivity)
      HIP_CHECK(hipMemcpyAsync(diffusivity, v->gdev, sizeof(double) * v->N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
  });
}

int mad_pm_gradient(mad_pm_ctx* v, const void* image, int32_t dtype, double* grad_soa) {
  if (!v || !image || !grad_soa) return MAD_ERR_INVALID;
  return pm_guarded(v, [&] {
    HIP_CHECK(hipSetDevice(v->mad->device));
    pm_load_image(v, image, dtype, false);
    double* G = nullptr;
    const size_t gbytes = sizeof(double) * v->C * v->dim * v->N;  // channel slowest
    HIP_CHECK(big_alloc((void**)&G, gbytes));
    std::unique_ptr<double, void (*)(double*)> hold(G, [](double* p) { (void)hipFree(p); });
    pm_generate_any(v, PM_GRADIENT, G, v->N, nullptr, nullptr);
    HIP_CHECK(hipMemcpyAsync(grad_soa, G, gbytes, hipMemcpyDeviceToHost, v->mad->stream));
    HIP_CHECK(hipStreamSynchronize(v->mad->stream));
  });
}

int mad_pm_contrast(mad_pm_ctx* v, const void* image, int32_t dtype, double q, double* contrast) {
  if (!v || !image || !contrast) return MAD_ERR_INVALID;
  return pm_guarded(v, [&] {
    REQUIRE(q > 0.0 && q <= 1.0, MAD_ERR_INVALID, "the quantile q must lie in (0, 1]");
    HIP_CHECK(hipSetDevice(v->mad->device));
    pm_load_image(v, image, dtype, false);
    pm_generate_any(v, PM_SQNORM, nullptr, v->N, nullptr, nullptr, q);
    HIP_CHECK(hipStreamSynchronize(v->mad->stream));
    *contrast = std::sqrt(v->k2_host[kK2Inspection]);
  });
}

int mad_pm_select(mad_pm_ctx* v, const double* values, int64_t n, int64_t k, double* out) {
  if (!v || !values || !out) return MAD_ERR_INVALID;
  return pm_guarded(v, [&] {
    REQUIRE(n >= 1 && k >= 0 && k < n, MAD_ERR_INVALID, "mad_pm_select needs n >= 1 and 0 <= k < n");
    HIP_CHECK(hipSetDevice(v->mad->device));
    pm_select_scratch(v, n, sizeof(uint64_t));
    hipStream_t st = v->mad->stream;
    void* keys = pm_stage(v, sizeof(double) * (size_t)n);
    HIP_CHECK(hipMemcpyAsync(keys, values, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_CHECK(select_launch<uint64_t>(v->sel, (const uint64_t*)keys, n, k, st));
    HIP_CHECK(hipMemcpyAsync(v->k2_host + kK2Inspection, v->sel.value(), sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    *out = v->k2_host[kK2Inspection];
  });
}

}  // extern "C"
