// C++ check of the indexed inputs of mad::PeronaMalikDiffusionImageFilter (include/mad_itk.hpp;
// mad_pm.h "Vector-valued images").
//   pm_vector_facade_test host -> no GPU: mad_pm_desc_init leaves channels 0 in a 176-byte
//                                 descriptor, the word follows contrast_mode, channel counts -1 and
//                                 17 are refused with a message, and the filter counts its inputs
//   pm_vector_facade_test run  -> two channels, a 2D int16 image and a 3D float image: a strong step
//                                 in channel 0 and a weak one under a ripple in channel 1; the
//                                 outputs keep size, spacing and origin, both channels change, equal
//                                 channels come out equal, and the weak step survives better than
//                                 through the scalar filter
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "mad_itk.hpp"

using Image2 = mad::itkshim::Image<int16_t, 2>;
using Image3 = mad::itkshim::Image<float, 3>;
using Filter2 = mad::PeronaMalikDiffusionImageFilter<Image2, Image2>;
using Filter3 = mad::PeronaMalikDiffusionImageFilter<Image3, Image3>;

static int host() {
  mad_pm_desc d;
  std::memset(&d, 0xA5, sizeof d);
  if (mad_pm_desc_init(&d) != MAD_OK) return 1;
  if (sizeof(mad_pm_desc) != 176 || d.channels != 0 || d.reserved[0] != 0 || d.reserved[1] != 0 || d.reserved[2] != 0)
    return 2;
  if (offsetof(mad_pm_desc, channels) != offsetof(mad_pm_desc, contrast_mode) + 4) return 3;
  d.channels = 3;
  if (d.reserved[0] != 3) return 4;  // the first of the three reserved words names it too
  for (int bad : {-1, 17}) {
    mad_pm_desc_init(&d);
    d.size[0] = 10, d.size[1] = 9, d.size[2] = 8;
    d.channels = bad;
    mad_pm_ctx* ctx = nullptr;
    const int rc = mad_pm_create(&d, &ctx);
    std::printf("channels %d: %d %s\n", bad, rc, mad_pm_last_error(nullptr));
    if (rc != MAD_ERR_INVALID || ctx || !std::strstr(mad_pm_last_error(nullptr), "channels")) return 5;
  }
  auto f = Filter2::New();
  auto a = Image2::New(), b = Image2::New();
  if (f->GetNumberOfChannels() != 1 || f->GetDescriptor().channels != 0) return 6;
  f->SetInput(a.get());
  f->SetInput(1, b.get());
  if (f->GetNumberOfChannels() != 2 || f->GetOutput(1)) return 7;
  std::printf("host ok\n");
  return 0;
}

// step: the height of the step at nx / 2; ripple: a fixed texture on top.  Rounded, so int16 holds it.
template <class Image>
static typename Image::Pointer make(const typename Image::SizeType& size, const typename Image::SpacingType& sp,
                                    double base, double step, double ripple) {
  auto img = Image::New();
  img->SetRegions(size);
  img->Allocate();
  img->SetSpacing(sp);
  typename Image::SpacingType origin{};
  for (unsigned q = 0; q < Image::ImageDimension; ++q) origin[q] = 1.0 + q;
  img->SetOrigin(origin);
  const int64_t nx = size[0];
  for (int64_t i = 0; i < img->NumberOfPixels(); ++i) {
    const int64_t x = i % nx, y = (i / nx) % size[1];
    const double v = std::floor(base + (x >= nx / 2 ? step : 0.0) + ripple * std::sin(2.9 * (double)x + 1.7 * (double)y));
    img->GetBufferPointer()[i] = (typename Image::PixelType)v;
  }
  return img;
}

// the mean jump across the step
template <class Image>
static double jump(const Image& img) {
  const int64_t nx = img.GetSize()[0], rows = img.NumberOfPixels() / nx;
  double s = 0.0;
  for (int64_t r = 0; r < rows; ++r)
    s += (double)img.GetBufferPointer()[r * nx + nx / 2] - (double)img.GetBufferPointer()[r * nx + nx / 2 - 1];
  return s / (double)rows;
}

template <class Filter>
static void configure(Filter& f) {
  f.SetDiffusivity(Filter::RATIONAL);
  f.SetNoiseScale(1.5);
  f.SetContrast(20.0);
  f.SetNumberOfIterations(2);
  f.SetDiffusionIterations(2);
  f.SetTimeStep(2.0);
}

template <class Filter, class Image>
static int run(const typename Image::SizeType& size, const typename Image::SpacingType& sp, const char* what) {
  // 4 x the behaviour test's amplitudes, so the integer pixels resolve the weak step
  auto strong = make<Image>(size, sp, 400.0, 200.0, 8.0), weak = make<Image>(size, sp, 40.0, 16.0, 8.0);
  auto f = Filter::New();
  configure(*f);
  f->SetInput(0, strong.get());
  f->SetInput(1, weak.get());
  f->Update();
  auto o0 = f->GetOutput(0), o1 = f->GetOutput(1);
  if (!o0 || !o1 || o0 != f->GetOutput() || f->GetOutput(2)) return 1;
  const mad_pm_stats st = f->GetStats();
  if (st.iterations != 2 || st.total_cycles < 2u * 2u * 2u || !f->GetConverged()) return 2;
  for (auto o : {o0, o1})
    if (o->GetSize() != size || o->GetSpacing() != sp || o->GetOrigin() != strong->GetOrigin()) return 3;
  bool changed0 = false, changed1 = false;
  for (int64_t i = 0; i < strong->NumberOfPixels(); ++i) {
    changed0 |= o0->GetBufferPointer()[i] != strong->GetBufferPointer()[i];
    changed1 |= o1->GetBufferPointer()[i] != weak->GetBufferPointer()[i];
  }
  if (!changed0 || !changed1) return 4;
  // the scalar filter on the weak channel alone
  auto s = Filter::New();
  configure(*s);
  s->SetInput(weak.get());
  s->Update();
  const double jin = jump(*weak), jjoint = jump(*o1), jsplit = jump(*s->GetOutput());
  std::printf("%s weak-step jump: input %.3f joint %.3f scalar %.3f; cycles %u\n", what, jin, jjoint, jsplit,
              st.total_cycles);
  if (!(jjoint > jsplit)) return 5;
  // equal channels come out equal
  auto e = Filter::New();
  configure(*e);
  e->SetInput(0, strong.get());
  e->SetInput(1, strong.get());
  e->Update();
  if (std::memcmp(e->GetOutput(0)->GetBufferPointer(), e->GetOutput(1)->GetBufferPointer(),
                  sizeof(typename Image::PixelType) * (size_t)strong->NumberOfPixels()) != 0)
    return 6;
  return 0;
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "run") == 0;
  if (!gpu) return host();
  if (int rc = run<Filter2, Image2>({40, 36}, {1.0, 1.0}, "2D int16")) return 10 + rc;
  if (int rc = run<Filter3, Image3>({24, 12, 10}, {1.0, 1.0, 1.0}, "3D float")) return 20 + rc;
  std::printf("run ok\n");
  return 0;
}
