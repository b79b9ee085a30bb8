// C++ drop-in check of mad::PeronaMalikDiffusionImageFilter (include/mad_itk.hpp), regularised
// Perona-Malik diffusion, in both dimensions.
//   pm_facade_test host -> no GPU: both dimensions compile, the defaults read back, the aliases
//                          set the same fields, and an invalid alpha and an unknown diffusivity
//                          are refused (mad_pm_create validates before it touches a device)
//   pm_facade_test run  -> a 2D int16 image and a 3D float image through the filter
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mad_itk.hpp"

using Image2 = mad::itkshim::Image<int16_t, 2>;
using Image3 = mad::itkshim::Image<float, 3>;
using Filter2 = mad::PeronaMalikDiffusionImageFilter<Image2, Image2>;
using Filter3 = mad::PeronaMalikDiffusionImageFilter<Image3, Image3, mad::MultigridGaussSeidelSmoother<3>>;

template <class Filter>
static bool defaults_ok() {
  auto f = Filter::New();
  const mad_pm_desc& d = f->GetDescriptor();
  return d.dim == 3 && d.diffusivity == MAD_PM_WEICKERT && d.noise_scale == 0.5 && d.contrast == 1.0 &&
         d.exponent == 2.0 && d.alpha == 0.01 && d.iterations == 1 && d.diffusion_iterations == 5 &&
         d.cycle == MAD_VCYCLE && d.time_step == 0.1 && d.tolerance == 1e-6 &&
         d.diffusion_iterations_per_grid == 2 && d.precision == MAD_PRECISION_AUTO && d.device == -1 &&
         f->GetConverged() && !f->GetOutput();
}

template <class Filter>
static bool aliases_ok() {
  auto f = Filter::New();
  f->SetConductanceParameter(3.5);
  f->SetNumberOfIterations(7);
  const mad_pm_desc& d = f->GetDescriptor();
  return d.contrast == 3.5 && d.iterations == 7;
}

template <class Filter, class Image>
static int invalid_throws(const Image* img, bool alpha) {
  auto f = Filter::New();
  f->SetInput(img);
  if (alpha) f->SetAlpha(1.5);
  else f->SetDiffusivity((typename Filter::DiffusivityType)3);
  try {
    f->Update();
  } catch (const mad::Error& e) {
    return e.code() == MAD_ERR_INVALID && std::strlen(e.what()) > std::strlen("mad_pm: ") ? 0 : 1;
  }
  return 1;
}

template <class Image>
static typename Image::Pointer make(const typename Image::SizeType& size, const typename Image::SpacingType& sp,
                                    const typename Image::SpacingType& origin) {
  auto img = Image::New();
  img->SetRegions(size);
  img->Allocate();
  img->SetSpacing(sp);
  img->SetOrigin(origin);
  const int64_t nx = size[0];
  for (int64_t i = 0; i < img->NumberOfPixels(); ++i) {
    const int64_t x = i % nx, y = (i / nx) % size[1];
    // a step along x with a ripple on top
    img->GetBufferPointer()[i] =
        (typename Image::PixelType)((x >= nx / 2 ? 150.0 : 100.0) + 4.0 * std::sin(0.9 * (double)x + 0.7 * (double)y));
  }
  return img;
}

template <class Filter, class Image>
static int run(const Image* img, typename Filter::DiffusivityType g, const char* what) {
  auto f = Filter::New();
  f->SetInput(img);
  f->SetDiffusivity(g);
  f->SetNoiseScale(0.7);
  f->SetConductanceParameter(5.0);
  f->SetExponent(2.0);
  f->SetAlpha(0.02);
  f->SetNumberOfIterations(2);
  f->SetDiffusionIterations(2);
  f->SetCycle(Filter::VCYCLE);
  f->SetTimeStep(0.2);
  f->SetTolerance(1e-6);
  f->SetDiffusionIterationsPerGrid(2);
  f->Update();
  auto out = f->GetOutput();
  static_assert(std::is_same<typename decltype(out)::element_type::PixelType, typename Image::PixelType>::value,
                "the output keeps its pixel type");
  if (out->GetSize() != img->GetSize() || out->GetSpacing() != img->GetSpacing() ||
      out->GetOrigin() != img->GetOrigin() || out->NumberOfPixels() != img->NumberOfPixels())
    return 1;
  const mad_pm_stats& st = f->GetStats();
  double sum = 0.0, moved = 0.0;
  for (int64_t i = 0; i < out->NumberOfPixels(); ++i) {
    sum += (double)out->GetBufferPointer()[i];
    moved += std::fabs((double)out->GetBufferPointer()[i] - (double)img->GetBufferPointer()[i]);
  }
  std::printf("%s cycles=%u relres=%.3e tensor_ms=%.4f pass0_ms=%.4f checksum=%.4f moved=%.4f\n", what,
              st.total_cycles, st.last_relres, st.tensor_ms, st.pass_ms[0], sum, moved);
  if (st.iterations != 2 || st.total_cycles < 4 || !(st.pass_ms[0] > 0.0) || !f->GetConverged()) return 2;
  if (Filter::Dim == 2 && (st.pass_ms[1] != 0.0 || st.pass_ms[2] != 0.0 || st.tile[0] <= 0)) return 3;
  if (Filter::Dim == 3 && (!(st.pass_ms[1] > 0.0) || !(st.pass_ms[2] > 0.0) || st.tile[0] != 0)) return 3;
  return moved > 0.0 ? 0 : 4;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "run") == 0;
  auto img2 = make<Image2>({40, 36}, {0.8, 1.25}, {1.0, 2.0});
  auto img3 = make<Image3>({20, 18, 12}, {0.8, 1.0, 1.25}, {1.0, 2.0, 3.0});
  if (!gpu) {
    if (!defaults_ok<Filter2>() || !defaults_ok<Filter3>()) return 2;
    if (!aliases_ok<Filter2>() || !aliases_ok<Filter3>()) return 3;
    for (bool alpha : {true, false})
      if (invalid_throws<Filter2>(img2.get(), alpha) || invalid_throws<Filter3>(img3.get(), alpha)) return 4;
    std::printf("host ok\n");
    return 0;
  }
  if (int rc = run<Filter2>(img2.get(), Filter2::RATIONAL, "2D int16")) return 10 + rc;
  if (int rc = run<Filter3>(img3.get(), Filter3::WEICKERT, "3D float")) return 20 + rc;
  std::printf("run ok\n");
  return 0;
}
