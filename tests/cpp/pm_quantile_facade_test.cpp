// C++ check of the contrast quantile of mad::PeronaMalikDiffusionImageFilter (include/mad_itk.hpp;
// mad_pm.h "Contrast from a quantile").
//   pm_quantile_facade_test host -> no GPU: the mode defaults to absolute, SetContrastQuantile and
//                                   SetContrast (and its alias) switch it, q = 0 and q > 1 are refused
//   pm_quantile_facade_test run  -> a 2D int16 image and a 3D float image in quantile mode: K is
//                                   reported, re-estimated in the second iteration, and scales by
//                                   exactly 4 with the image; mad_pm_contrast gives the same K
#include <cmath>
#include <cstdio>
#include <cstring>

#include "mad_itk.hpp"
#include "mad_pm_quantile.h"

using Image2 = mad::itkshim::Image<int16_t, 2>;
using Image3 = mad::itkshim::Image<float, 3>;
using Filter2 = mad::PeronaMalikDiffusionImageFilter<Image2, Image2>;
using Filter3 = mad::PeronaMalikDiffusionImageFilter<Image3, Image3>;

template <class Filter>
static bool modes_ok() {
  auto f = Filter::New();
  const mad_pm_desc& d = f->GetDescriptor();
  if (d.contrast_mode != MAD_PM_CONTRAST_ABSOLUTE || d.contrast != 1.0 || f->GetContrastUsed() != 0.0) return false;
  f->SetContrastQuantile(0.9);
  if (d.contrast_mode != MAD_PM_CONTRAST_QUANTILE || d.contrast != 0.9) return false;
  f->SetContrast(4.0);
  if (d.contrast_mode != MAD_PM_CONTRAST_ABSOLUTE || d.contrast != 4.0) return false;
  f->SetContrastQuantile(0.5);
  f->SetConductanceParameter(3.0);
  return d.contrast_mode == MAD_PM_CONTRAST_ABSOLUTE && d.contrast == 3.0;
}

template <class Filter, class Image>
static int invalid_throws(const Image* img, double q) {
  auto f = Filter::New();
  f->SetInput(img);
  f->SetContrastQuantile(q);
  try {
    f->Update();
  } catch (const mad::Error& e) {
    return e.code() == MAD_ERR_INVALID && std::strlen(e.what()) > std::strlen("mad_pm: ") ? 0 : 1;
  }
  return 1;
}

template <class Image>
static typename Image::Pointer make(const typename Image::SizeType& size, const typename Image::SpacingType& sp,
                                    double scale) {
  auto img = Image::New();
  img->SetRegions(size);
  img->Allocate();
  img->SetSpacing(sp);
  const int64_t nx = size[0];
  for (int64_t i = 0; i < img->NumberOfPixels(); ++i) {
    const int64_t x = i % nx, y = (i / nx) % size[1];
    // a step along x with a ripple on top, rounded so that int16 holds it and 4 x is exact
    const double v = std::floor((x >= nx / 2 ? 150.0 : 100.0) + 4.0 * std::sin(0.9 * (double)x + 0.7 * (double)y));
    img->GetBufferPointer()[i] = (typename Image::PixelType)(scale * v);
  }
  return img;
}

template <class Filter, class Image>
static double contrast_used(const Image* img, unsigned iterations, int* rc) {
  auto f = Filter::New();
  f->SetInput(img);
  f->SetNoiseScale(1.0);
  f->SetContrastQuantile(0.9);
  f->SetNumberOfIterations(iterations);
  f->SetDiffusionIterations(2);
  f->SetTimeStep(0.5);
  f->Update();
  if (f->GetStats().iterations != iterations || f->GetStats().contrast_used != f->GetContrastUsed()) *rc = 1;
  return f->GetContrastUsed();
}

template <class Filter, class Image>
static int run(const typename Image::SizeType& size, const typename Image::SpacingType& sp, const char* what) {
  auto img = make<Image>(size, sp, 1.0), img4 = make<Image>(size, sp, 4.0);
  int rc = 0;
  const double K1 = contrast_used<Filter>(img.get(), 1, &rc), K2 = contrast_used<Filter>(img.get(), 2, &rc);
  const double K4 = contrast_used<Filter>(img4.get(), 1, &rc);
  // the same K from the inspection entry point, on an absolute-mode context of the same parameters
  mad_pm_desc d;
  mad_pm_desc_init(&d);
  d.dim = (int32_t)Filter::Dim;
  for (unsigned q = 0; q < Filter::Dim; ++q) {
    d.size[q] = size[q];
    d.spacing[q] = sp[q];
  }
  d.noise_scale = 1.0;
  mad_pm_ctx* ctx = nullptr;
  double K = -1.0;
  if (mad_pm_create(&d, &ctx) != MAD_OK) return 2;
  const int crc = mad_pm_contrast(ctx, img->GetBufferPointer(), mad::itkshim::PixelTraits<typename Image::PixelType>::id,
                                  0.9, &K);
  mad_pm_destroy(ctx);
  std::printf("%s K=%.6f K(2 iterations)=%.6f K(4 u)=%.6f mad_pm_contrast=%.6f\n", what, K1, K2, K4, K);
  if (rc || crc != MAD_OK) return 3;
  // no iteration, no tensor generation: an identity run that reports K = 0
  if (contrast_used<Filter>(img.get(), 0, &rc) != 0.0 || rc) return 7;
  if (!(K1 > 0.0) || !(K2 > 0.0) || K2 == K1) return 4;  // re-estimated from the iterate
  if (K4 != 4.0 * K1) return 5;                            // scale covariance, exactly
  return K == K1 ? 0 : 6;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "run") == 0;
  if (!gpu) {
    if (!modes_ok<Filter2>() || !modes_ok<Filter3>()) return 2;
    auto img2 = make<Image2>({40, 36}, {0.8, 1.25}, 1.0);
    auto img3 = make<Image3>({20, 18, 12}, {0.8, 1.0, 1.25}, 1.0);
    for (double q : {0.0, 1.5, -0.25})
      if (invalid_throws<Filter2>(img2.get(), q) || invalid_throws<Filter3>(img3.get(), q)) return 3;
    std::printf("host ok\n");
    return 0;
  }
  if (int rc = run<Filter2, Image2>({40, 36}, {0.8, 1.25}, "2D int16")) return 10 + rc;
  if (int rc = run<Filter3, Image3>({20, 18, 12}, {0.8, 1.0, 1.25}, "3D float")) return 20 + rc;
  std::printf("run ok\n");
  return 0;
}
