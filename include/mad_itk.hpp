// mad_itk.hpp -- header-only, ITK-shaped C++ facade over the C ABI (mad.h).
//
// Mirrors the reference's filter surface so call sites port verbatim:
//   itk::MultigridAnisotropicDiffusionImageFilter<TIn, TOut, TSmoother>
//     include/itkMultigridAnisotropicDiffusionImageFilter.h:89-160
//   smoother plug-ins  mad::MultigridGaussSeidelSmoother<D> / MultigridWeightedJacobiSmoother<D>
//     include/mad/itkMultigridGaussSeidelSmoother.h, itkMultigridWeightedJacobiSmoother.h
//   itk::VEDMultigridImageFilter<TIn, TOut, TSmoother>
//     include/itkVEDMultigridImageFilter.h:43-168 (through mad_ved.h)
//   mad::CoherenceEnhancingDiffusionImageFilter<TIn, TOut, TSmoother>
//     structure-tensor EED / CED, 2D or 3D (through mad_ced.h; the setter names of ITK's
//     AnisotropicDiffusionLBR filter of that name)
//   mad::PeronaMalikDiffusionImageFilter<TIn, TOut, TSmoother>
//     regularised Perona-Malik diffusion, 2D or 3D (through mad_pm.h; SetConductanceParameter /
//     SetNumberOfIterations as in ITK's anisotropic-diffusion family)
// ITK itself is not a dependency: images are the small mad::itkshim::Image below
// (buffer + size + spacing + origin, x fastest, region index 0).  With a real
// ITK build the same class body sits behind itk::ImageToImageFilter: GenerateData
// forwards GetInput()->GetBufferPointer() etc. to Run().
#ifndef MAD_ITK_HPP
#define MAD_ITK_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "mad.h"
#include "mad_ced.h"
#include "mad_pm.h"
#include "mad_ved.h"

namespace mad {
namespace itkshim {

template <typename T>
struct PixelTraits;
template <> struct PixelTraits<uint8_t> { static constexpr int32_t id = MAD_U8; };
template <> struct PixelTraits<int8_t> { static constexpr int32_t id = MAD_I8; };
template <> struct PixelTraits<uint16_t> { static constexpr int32_t id = MAD_U16; };
template <> struct PixelTraits<int16_t> { static constexpr int32_t id = MAD_I16; };
template <> struct PixelTraits<uint32_t> { static constexpr int32_t id = MAD_U32; };
template <> struct PixelTraits<int32_t> { static constexpr int32_t id = MAD_I32; };
template <> struct PixelTraits<float> { static constexpr int32_t id = MAD_F32; };
template <> struct PixelTraits<double> { static constexpr int32_t id = MAD_F64; };

// itk::Image<TPixel, VDim> stand-in (LargestPossibleRegion with index 0)
template <typename TPixel, unsigned int VDim>
class Image {
 public:
  using PixelType = TPixel;
  static constexpr unsigned int ImageDimension = VDim;
  using Pointer = std::shared_ptr<Image>;
  using SizeType = std::array<int64_t, VDim>;
  using SpacingType = std::array<double, VDim>;

  static Pointer New() { return std::make_shared<Image>(); }
  void SetRegions(const SizeType& s) { size_ = s; }
  void Allocate() {
    int64_t n = 1;
    for (auto v : size_) n *= v;
    buf_.assign((size_t)n, TPixel());
  }
  void SetSpacing(const SpacingType& s) { spacing_ = s; }
  void SetOrigin(const SpacingType& o) { origin_ = o; }
  const SizeType& GetSize() const { return size_; }
  const SpacingType& GetSpacing() const { return spacing_; }
  const SpacingType& GetOrigin() const { return origin_; }
  TPixel* GetBufferPointer() { return buf_.data(); }
  const TPixel* GetBufferPointer() const { return buf_.data(); }
  int64_t NumberOfPixels() const { return (int64_t)buf_.size(); }

 private:
  SizeType size_{};
  SpacingType spacing_{};
  SpacingType origin_{};
  std::vector<TPixel> buf_;
};

// itk::SymmetricSecondRankTensor<T, D>: D(D+1)/2 components, ITK order
template <typename T, unsigned int VDim>
struct SymmetricSecondRankTensor {
  std::array<T, VDim * (VDim + 1) / 2> c{};
  T& operator()(unsigned r, unsigned q) {
    if (r > q) std::swap(r, q);
    return c[r * VDim - r * (r - 1) / 2 + (q - r)];
  }
};

}  // namespace itkshim

// smoother plug-ins (template argument TSmootherType)
template <unsigned int VDim>
struct MultigridGaussSeidelSmoother {
  static constexpr int32_t id = MAD_GAUSS_SEIDEL;
};
template <unsigned int VDim>
struct MultigridGaussSeidelLexSmoother {
  static constexpr int32_t id = MAD_GAUSS_SEIDEL_LEX;
};
template <unsigned int VDim>
struct MultigridWeightedJacobiSmoother {
  static constexpr int32_t id = MAD_WEIGHTED_JACOBI;
};

class Error : public std::runtime_error {
 public:
  Error(int code, const std::string& m) : std::runtime_error(m), code_(code) {}
  int code() const { return code_; }

 private:
  int code_;
};

inline void check(int rc, const mad_ctx* c = nullptr) {
  if (rc != MAD_OK) throw Error(rc, std::string("mad: ") + mad_last_error(c));
}

// MAD_ERR_NOT_CONVERGED is a warning (the output is written), as an ITK filter would report it
// with itkWarningMacro instead of an exception; returns false then
inline bool check_run(int rc, const char* what, const char* msg) {
  if (rc == MAD_ERR_NOT_CONVERGED) {
    std::cerr << "WARNING: " << what << ": " << msg << std::endl;
    return false;
  }
  if (rc != MAD_OK) throw Error(rc, std::string(what) + ": " + msg);
  return true;
}

template <class TInputImage, class TOutputImage,
          class TSmootherType = MultigridGaussSeidelSmoother<TInputImage::ImageDimension>>
class MultigridAnisotropicDiffusionImageFilter {
 public:
  using Self = MultigridAnisotropicDiffusionImageFilter;
  using Pointer = std::shared_ptr<Self>;
  using InputPixelType = typename TInputImage::PixelType;
  using OutputPixelType = typename TOutputImage::PixelType;
  static constexpr unsigned int Dim = TInputImage::ImageDimension;
  using InputTensorImageType =
      itkshim::Image<itkshim::SymmetricSecondRankTensor<InputPixelType, Dim>, Dim>;
  using Precision = double;
  enum CycleType { VCYCLE = MAD_VCYCLE, FMG = MAD_FMG, SMOOTHER = MAD_SMOOTHER };  // .h:123

  static Pointer New() { return Pointer(new Self()); }
  ~MultigridAnisotropicDiffusionImageFilter() { mad_destroy(ctx_); }

  // setters (.h:133-160)
  void SetCycle(CycleType c) { desc_.cycle = c; }
  void SetIterationsPerGrid(unsigned int n) { desc_.iterations_per_grid = n; }
  void SetMaxCycles(unsigned int n) { desc_.max_cycles = n; }
  void SetNumberOfSteps(unsigned int n) { desc_.number_of_steps = n; }
  void SetTimeStep(Precision dt) { desc_.time_step = dt; }
  void SetTolerance(Precision t) { desc_.tolerance = t; }
  void SetVerbose(bool v) { desc_.verbose = v ? 1 : 0; }
  // MI355X execution options (no reference counterpart)
  void SetPrecision(int32_t p) { desc_.precision = p; desc_.stall_guard = (p != MAD_FP64); }
  void SetDevice(int32_t d) { desc_.device = d; }
  // the reference's -DBENCHMARK build (.hxx:145-151, 222-227, 401-409, 450-458, 477-485): Update()
  // records the relres / seconds history (MAD_OPT_BENCHMARK_TRACE) and writes it to benchmark.txt as
  // "relres_seconds" lines.  On by default when this header is compiled with -DBENCHMARK, as there.
  void SetBenchmark(bool on) {
    desc_.options = on ? (desc_.options | MAD_OPT_BENCHMARK_TRACE) : (desc_.options & ~MAD_OPT_BENCHMARK_TRACE);
  }
  // the history of the last Update() with SetBenchmark(true), one "relres_seconds" line per entry
  std::vector<std::string> GetBenchmarkOutput() const { return bench_; }

  // SetDiffusionTensor (.hxx:66-101): copied and cast to fp64 at call time
  void SetDiffusionTensor(const InputTensorImageType* t) {
    const int64_t n = t->NumberOfPixels();
    constexpr int nc = Dim * (Dim + 1) / 2;
    tensor_.resize((size_t)n * nc);
    const auto* src = t->GetBufferPointer();
    for (int64_t p = 0; p < n; ++p)
      for (int c = 0; c < nc; ++c) tensor_[(size_t)p * nc + c] = (double)src[p].c[c];
  }
  void SetInput(const TInputImage* img) { input_ = img; }
  typename TOutputImage::Pointer GetOutput() const { return output_; }
  const mad_stats& GetStats() const { return stats_; }

  // GenerateData (.hxx:104-297), on the GPU through mad_run
  void Update() {
    if (!input_ || tensor_.empty()) throw Error(MAD_ERR_STATE, "SetInput and SetDiffusionTensor first");
    mad_desc d = desc_;
    d.dim = (int32_t)Dim;
    for (unsigned q = 0; q < 3; ++q) {
      d.size[q] = q < Dim ? input_->GetSize()[q] : 1;
      d.spacing[q] = q < Dim ? input_->GetSpacing()[q] : 1.0;
    }
    d.smoother = TSmootherType::id;
    mad_destroy(ctx_);
    ctx_ = nullptr;
    check(mad_create(&d, &ctx_));
    check(mad_set_tensor(ctx_, tensor_.data(), MAD_F64), ctx_);
    output_ = TOutputImage::New();
    output_->SetRegions(input_->GetSize());
    output_->Allocate();
    output_->SetSpacing(input_->GetSpacing());
    output_->SetOrigin(input_->GetOrigin());  // .hxx:286
    const int rc = mad_run(ctx_, input_->GetBufferPointer(), itkshim::PixelTraits<InputPixelType>::id,
                           output_->GetBufferPointer(), itkshim::PixelTraits<OutputPixelType>::id, &stats_);
    converged_ = check_run(rc, "mad", mad_last_error(ctx_));
    bench_.clear();
    if (d.options & MAD_OPT_BENCHMARK_TRACE) {
      uint32_t n = 0;
      check(mad_get_cycle_trace(ctx_, 0, nullptr, nullptr, nullptr, &n), ctx_);
      std::vector<double> rr(n), sec(n);
      check(mad_get_cycle_trace(ctx_, n, nullptr, rr.data(), sec.data(), &n), ctx_);
      std::ofstream f("benchmark.txt");  // m_BenchmarkOutput.open("benchmark.txt"), .hxx:147
      for (uint32_t q = 0; q < n; ++q) {
        std::ostringstream ln;
        ln << rr[q] << "_" << (float)sec[q];  // .hxx:225: relres << "_" << (float) seconds
        bench_.push_back(ln.str());
        f << bench_.back() << std::endl;
      }
    }
  }
  // false when the stall guard ended a time step above the tolerance (MAD_ERR_NOT_CONVERGED)
  bool GetConverged() const { return converged_; }

 protected:
  MultigridAnisotropicDiffusionImageFilter() {
    check(mad_desc_init(&desc_));
#ifdef BENCHMARK
    SetBenchmark(true);
#endif
  }

 private:
  mad_desc desc_{};
  std::vector<std::string> bench_;
  mad_ctx* ctx_ = nullptr;
  mad_stats stats_{};
  bool converged_ = true;
  const TInputImage* input_ = nullptr;
  std::vector<double> tensor_;
  typename TOutputImage::Pointer output_;
};

// itk::VEDMultigridImageFilter (VED.h:43-168): vessel enhancing diffusion, the caller of
// the multigrid filter; the whole pipeline runs on the GPU through mad_ved.h.
template <class TInputImage, class TOutputImage,
          class TSmootherType = MultigridGaussSeidelSmoother<TInputImage::ImageDimension>>
class VEDMultigridImageFilter {
 public:
  static_assert(TInputImage::ImageDimension == 3, "VED is 3D (VED.h:46)");
  using Self = VEDMultigridImageFilter;
  using Pointer = std::shared_ptr<Self>;
  using InputPixelType = typename TInputImage::PixelType;
  using OutputPixelType = typename TOutputImage::PixelType;
  using Precision = double;
  enum CycleType { VCYCLE = MAD_VCYCLE, FMG = MAD_FMG, SMOOTHER = MAD_SMOOTHER };

  static Pointer New() { return Pointer(new Self()); }
  ~VEDMultigridImageFilter() { mad_ved_destroy(ctx_); }

  // setters (VED.h:88-106)
  void SetAlpha(Precision v) { desc_.alpha = v; }
  void SetBeta(Precision v) { desc_.beta = v; }
  void SetGamma(Precision v) { desc_.gamma = v; }
  void SetEpsilon(Precision v) { desc_.epsilon = v; }
  void SetOmega(Precision v) { desc_.omega = v; }
  void SetSensitivity(Precision v) { desc_.sensitivity = v; }
  void SetScales(const std::vector<Precision>& s) {
    if (s.empty() || s.size() > MAD_VED_MAX_SCALES) throw Error(MAD_ERR_INVALID, "1..16 scales");
    desc_.nscales = (int32_t)s.size();
    for (size_t q = 0; q < s.size(); ++q) desc_.scales[q] = s[q];
  }
  void SetIterations(unsigned int n) { desc_.iterations = n; }
  void SetDiffusionIterations(unsigned int n) { desc_.diffusion_iterations = n; }
  void SetCycle(CycleType c) { desc_.cycle = c; }
  void SetTimeStep(Precision dt) { desc_.time_step = dt; }
  void SetTolerance(Precision t) { desc_.tolerance = t; }
  void SetDiffusionIterationsPerGrid(unsigned int n) { desc_.diffusion_iterations_per_grid = n; }
  void SetVerbose(bool v) { desc_.verbose = v ? 1 : 0; }
  // MI355X execution options (no reference counterpart)
  void SetPrecision(int32_t p) { desc_.precision = p; }
  void SetDevice(int32_t d) { desc_.device = d; }

  void SetInput(const TInputImage* img) { input_ = img; }
  typename TOutputImage::Pointer GetOutput() const { return output_; }
  const mad_ved_stats& GetStats() const { return stats_; }

  // GenerateData (VED.hxx:63-155)
  void Update() {
    if (!input_) throw Error(MAD_ERR_STATE, "SetInput first");
    mad_ved_desc d = desc_;
    for (unsigned q = 0; q < 3; ++q) {
      d.size[q] = input_->GetSize()[q];
      d.spacing[q] = input_->GetSpacing()[q];
    }
    d.smoother = TSmootherType::id;
    mad_ved_destroy(ctx_);
    ctx_ = nullptr;
    if (int rc = mad_ved_create(&d, &ctx_))
      throw Error(rc, std::string("mad_ved: ") + mad_ved_last_error(nullptr));
    output_ = TOutputImage::New();
    output_->SetRegions(input_->GetSize());
    output_->Allocate();
    output_->SetSpacing(input_->GetSpacing());
    output_->SetOrigin(input_->GetOrigin());
    const int rc = mad_ved_run(ctx_, input_->GetBufferPointer(), itkshim::PixelTraits<InputPixelType>::id,
                               output_->GetBufferPointer(), itkshim::PixelTraits<OutputPixelType>::id,
                               &stats_);
    converged_ = check_run(rc, "mad_ved", mad_ved_last_error(ctx_));
  }
  bool GetConverged() const { return converged_; }

 protected:
  VEDMultigridImageFilter() { check(mad_ved_desc_init(&desc_)); }

 private:
  mad_ved_desc desc_{};
  mad_ved_ctx* ctx_ = nullptr;
  mad_ved_stats stats_{};
  bool converged_ = true;
  const TInputImage* input_ = nullptr;
  typename TOutputImage::Pointer output_;
};

// Structure-tensor diffusion (Weickert's EED / CED, mad_ced.h): the tensor comes from the image
// itself, so there is no SetDiffusionTensor.  Templated on the dimension like ITK's
// CoherenceEnhancingDiffusionImageFilter: a 2D image takes the fused 2D tensor kernel
// (mad_ced_desc.dim = 2), a 3D image the five passes.
template <class TInputImage, class TOutputImage,
          class TSmootherType = MultigridGaussSeidelSmoother<TInputImage::ImageDimension>>
class CoherenceEnhancingDiffusionImageFilter {
 public:
  static constexpr unsigned int Dim = TInputImage::ImageDimension;
  static_assert(Dim == 2 || Dim == 3, "structure-tensor diffusion is 2D or 3D");
  static_assert(TOutputImage::ImageDimension == Dim, "input and output dimensions differ");
  using Self = CoherenceEnhancingDiffusionImageFilter;
  using Pointer = std::shared_ptr<Self>;
  using InputPixelType = typename TInputImage::PixelType;
  using OutputPixelType = typename TOutputImage::PixelType;
  using Precision = double;
  enum CycleType { VCYCLE = MAD_VCYCLE, FMG = MAD_FMG, SMOOTHER = MAD_SMOOTHER };
  enum EnhancementType { EED = MAD_CED_EED, CED = MAD_CED_CED };

  static Pointer New() { return Pointer(new Self()); }
  ~CoherenceEnhancingDiffusionImageFilter() { mad_ced_destroy(ctx_); }

  void SetEnhancement(EnhancementType e) { desc_.enhancement = e; }
  void SetNoiseScale(Precision v) { desc_.noise_scale = v; }
  void SetFeatureScale(Precision v) { desc_.feature_scale = v; }
  void SetContrast(Precision v) { desc_.contrast = v; }
  void SetExponent(Precision v) { desc_.exponent = v; }
  void SetAlpha(Precision v) { desc_.alpha = v; }
  void SetIterations(unsigned int n) { desc_.iterations = n; }
  void SetDiffusionIterations(unsigned int n) { desc_.diffusion_iterations = n; }
  void SetCycle(CycleType c) { desc_.cycle = c; }
  void SetTimeStep(Precision dt) { desc_.time_step = dt; }
  void SetTolerance(Precision t) { desc_.tolerance = t; }
  void SetDiffusionIterationsPerGrid(unsigned int n) { desc_.diffusion_iterations_per_grid = n; }
  void SetVerbose(bool v) { desc_.verbose = v ? 1 : 0; }
  // MI355X execution options
  void SetPrecision(int32_t p) { desc_.precision = p; }
  void SetDevice(int32_t d) { desc_.device = d; }

  const mad_ced_desc& GetDescriptor() const { return desc_; }
  void SetInput(const TInputImage* img) { input_ = img; }
  typename TOutputImage::Pointer GetOutput() const { return output_; }
  const mad_ced_stats& GetStats() const { return stats_; }

  void Update() {
    if (!input_) throw Error(MAD_ERR_STATE, "SetInput first");
    mad_ced_desc d = desc_;
    d.dim = (int32_t)Dim;
    for (unsigned q = 0; q < 3; ++q) {
      d.size[q] = q < Dim ? input_->GetSize()[q] : 1;
      d.spacing[q] = q < Dim ? input_->GetSpacing()[q] : 1.0;
    }
    d.smoother = TSmootherType::id;
    mad_ced_destroy(ctx_);
    ctx_ = nullptr;
    if (int rc = mad_ced_create(&d, &ctx_))
      throw Error(rc, std::string("mad_ced: ") + mad_ced_last_error(nullptr));
    output_ = TOutputImage::New();
    output_->SetRegions(input_->GetSize());
    output_->Allocate();
    output_->SetSpacing(input_->GetSpacing());
    output_->SetOrigin(input_->GetOrigin());
    const int rc = mad_ced_run(ctx_, input_->GetBufferPointer(), itkshim::PixelTraits<InputPixelType>::id,
                               output_->GetBufferPointer(), itkshim::PixelTraits<OutputPixelType>::id,
                               &stats_);
    converged_ = check_run(rc, "mad_ced", mad_ced_last_error(ctx_));
  }
  bool GetConverged() const { return converged_; }

 protected:
  CoherenceEnhancingDiffusionImageFilter() {
    if (int rc = mad_ced_desc_init(&desc_)) throw Error(rc, "mad_ced_desc_init");
  }

 private:
  mad_ced_desc desc_{};
  mad_ced_ctx* ctx_ = nullptr;
  mad_ced_stats stats_{};
  bool converged_ = true;
  const TInputImage* input_ = nullptr;
  typename TOutputImage::Pointer output_;
};

// Regularised Perona-Malik diffusion (mad_pm.h): D = g I with a scalar diffusivity of the
// squared gradient at the noise scale.  Templated on the dimension like the filter above: a 2D
// image takes the fused 2D tensor kernel (mad_pm_desc.dim = 2), a 3D image the three passes.
// SetConductanceParameter / SetNumberOfIterations, the names of ITK's anisotropic-diffusion
// family, are aliases of SetContrast / SetIterations; the implicit steps take time steps of
// 1-10 where those explicit filters are capped near 0.06-0.125.
template <class TInputImage, class TOutputImage,
          class TSmootherType = MultigridGaussSeidelSmoother<TInputImage::ImageDimension>>
class PeronaMalikDiffusionImageFilter {
 public:
  static constexpr unsigned int Dim = TInputImage::ImageDimension;
  static_assert(Dim == 2 || Dim == 3, "Perona-Malik diffusion is 2D or 3D");
  static_assert(TOutputImage::ImageDimension == Dim, "input and output dimensions differ");
  using Self = PeronaMalikDiffusionImageFilter;
  using Pointer = std::shared_ptr<Self>;
  using InputPixelType = typename TInputImage::PixelType;
  using OutputPixelType = typename TOutputImage::PixelType;
  using Precision = double;
  enum CycleType { VCYCLE = MAD_VCYCLE, FMG = MAD_FMG, SMOOTHER = MAD_SMOOTHER };
  enum DiffusivityType {
    WEICKERT = MAD_PM_WEICKERT,
    EXPONENTIAL = MAD_PM_EXPONENTIAL,
    RATIONAL = MAD_PM_RATIONAL
  };

  static Pointer New() { return Pointer(new Self()); }
  ~PeronaMalikDiffusionImageFilter() { mad_pm_destroy(ctx_); }

  void SetDiffusivity(DiffusivityType g) { desc_.diffusivity = g; }
  void SetNoiseScale(Precision v) { desc_.noise_scale = v; }
  // an absolute contrast K (leaves quantile mode)
  void SetContrast(Precision v) {
    desc_.contrast = v;
    desc_.contrast_mode = MAD_PM_CONTRAST_ABSOLUTE;
  }
  void SetConductanceParameter(Precision v) { SetContrast(v); }
  // K from the q-quantile of the gradient magnitudes, selected on the device in every iteration
  // (0 < q <= 1; Perona and Malik: 0.9): mad_pm.h, "Contrast from a quantile"
  void SetContrastQuantile(Precision q) {
    desc_.contrast = q;
    desc_.contrast_mode = MAD_PM_CONTRAST_QUANTILE;
  }
  // K of the last tensor generation of the last Update (0 before it)
  Precision GetContrastUsed() const { return stats_.contrast_used; }
  void SetExponent(Precision v) { desc_.exponent = v; }
  void SetAlpha(Precision v) { desc_.alpha = v; }
  void SetIterations(unsigned int n) { desc_.iterations = n; }
  void SetNumberOfIterations(unsigned int n) { SetIterations(n); }
  void SetDiffusionIterations(unsigned int n) { desc_.diffusion_iterations = n; }
  void SetCycle(CycleType c) { desc_.cycle = c; }
  void SetTimeStep(Precision dt) { desc_.time_step = dt; }
  void SetTolerance(Precision t) { desc_.tolerance = t; }
  void SetDiffusionIterationsPerGrid(unsigned int n) { desc_.diffusion_iterations_per_grid = n; }
  void SetVerbose(bool v) { desc_.verbose = v ? 1 : 0; }
  // MI355X execution options
  void SetPrecision(int32_t p) { desc_.precision = p; }
  void SetDevice(int32_t d) { desc_.device = d; }

  const mad_pm_desc& GetDescriptor() const { return desc_; }
  void SetInput(const TInputImage* img) { input_ = img; }
  typename TOutputImage::Pointer GetOutput() const { return output_; }
  const mad_pm_stats& GetStats() const { return stats_; }

  // Vector-valued images (mad_pm.h "Vector-valued images"), ITK's indexed inputs: channel c of
  // the image is input c, its output GetOutput(c); one joint diffusivity for all.  Channels must
  // be set without gaps from 0 and share their size.  SetInput(img) is SetInput(0, img) and
  // GetOutput() is GetOutput(0); spacing and origin are channel 0's.
  void SetInput(unsigned int c, const TInputImage* img) {
    if (c == 0) input_ = img;
    if (c > 0 && more_.size() < c) more_.resize(c, nullptr);
    if (c > 0) more_[c - 1] = img;
  }
  typename TOutputImage::Pointer GetOutput(unsigned int c) const {
    return c == 0 ? output_ : c <= more_out_.size() ? more_out_[c - 1] : nullptr;
  }
  unsigned int GetNumberOfChannels() const { return 1 + (unsigned int)more_.size(); }

  void Update() {
    if (!input_) throw Error(MAD_ERR_STATE, "SetInput first");
    if (!more_.empty()) return UpdateChannels();
    mad_pm_desc d = desc_;
    d.dim = (int32_t)Dim;
    for (unsigned q = 0; q < 3; ++q) {
      d.size[q] = q < Dim ? input_->GetSize()[q] : 1;
      d.spacing[q] = q < Dim ? input_->GetSpacing()[q] : 1.0;
    }
    d.smoother = TSmootherType::id;
    mad_pm_destroy(ctx_);
    ctx_ = nullptr;
    if (int rc = mad_pm_create(&d, &ctx_))
      throw Error(rc, std::string("mad_pm: ") + mad_pm_last_error(nullptr));
    output_ = TOutputImage::New();
    output_->SetRegions(input_->GetSize());
    output_->Allocate();
    output_->SetSpacing(input_->GetSpacing());
    output_->SetOrigin(input_->GetOrigin());
    const int rc = mad_pm_run(ctx_, input_->GetBufferPointer(), itkshim::PixelTraits<InputPixelType>::id,
                              output_->GetBufferPointer(), itkshim::PixelTraits<OutputPixelType>::id,
                              &stats_);
    converged_ = check_run(rc, "mad_pm", mad_pm_last_error(ctx_));
  }
  bool GetConverged() const { return converged_; }

 protected:
  PeronaMalikDiffusionImageFilter() {
    if (int rc = mad_pm_desc_init(&desc_)) throw Error(rc, "mad_pm_desc_init");
  }

 private:
  // more than one channel: packs the channel buffers planar (channel c at element offset c N),
  // sets desc.channels, and unpacks the planar output into one image per channel
  void UpdateChannels() {
    const unsigned C = GetNumberOfChannels();
    const int64_t N = input_->NumberOfPixels();
    std::vector<InputPixelType> in((size_t)(C * N));
    for (unsigned c = 0; c < C; ++c) {
      const TInputImage* img = c == 0 ? input_ : more_[c - 1];
      if (!img) throw Error(MAD_ERR_STATE, "SetInput(c, image): a channel below the last one is missing");
      if (img->GetSize() != input_->GetSize()) throw Error(MAD_ERR_INVALID, "the channels differ in size");
      std::copy(img->GetBufferPointer(), img->GetBufferPointer() + N, in.begin() + (size_t)c * N);
    }
    mad_pm_desc d = desc_;
    d.dim = (int32_t)Dim;
    d.channels = (int32_t)C;
    for (unsigned q = 0; q < 3; ++q) {
      d.size[q] = q < Dim ? input_->GetSize()[q] : 1;
      d.spacing[q] = q < Dim ? input_->GetSpacing()[q] : 1.0;
    }
    d.smoother = TSmootherType::id;
    mad_pm_destroy(ctx_);
    ctx_ = nullptr;
    if (int rc = mad_pm_create(&d, &ctx_))
      throw Error(rc, std::string("mad_pm: ") + mad_pm_last_error(nullptr));
    std::vector<OutputPixelType> out((size_t)(C * N));
    const int rc = mad_pm_run(ctx_, in.data(), itkshim::PixelTraits<InputPixelType>::id, out.data(),
                              itkshim::PixelTraits<OutputPixelType>::id, &stats_);
    converged_ = check_run(rc, "mad_pm", mad_pm_last_error(ctx_));  // throws unless the output is written
    more_out_.assign(C - 1, nullptr);
    for (unsigned c = 0; c < C; ++c) {
      auto o = TOutputImage::New();
      o->SetRegions(input_->GetSize());
      o->Allocate();
      o->SetSpacing(input_->GetSpacing());
      o->SetOrigin(input_->GetOrigin());
      std::copy(out.begin() + (size_t)c * N, out.begin() + (size_t)(c + 1) * N, o->GetBufferPointer());
      (c == 0 ? output_ : more_out_[c - 1]) = o;
    }
  }

  mad_pm_desc desc_{};
  mad_pm_ctx* ctx_ = nullptr;
  mad_pm_stats stats_{};
  bool converged_ = true;
  const TInputImage* input_ = nullptr;
  typename TOutputImage::Pointer output_;
  std::vector<const TInputImage*> more_;                    // channels 1..
  std::vector<typename TOutputImage::Pointer> more_out_;
};

}  // namespace mad
#endif  // MAD_ITK_HPP
