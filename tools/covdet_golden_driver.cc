// covdet_golden_driver.cc -- runs VLFeat's covdet over one grey image in the call sequence of COLMAP's
// ExtractCovariantSiftFeaturesCPU with estimate_affine_shape = false (src/feature/sift.cc:440-573) and writes what VLFeat
// returned, untouched: the features after detection (a second detector with the non-extrema suppression switched off),
// after the suppression, after the orientations, after COLMAP's std::sort, and VlFeat's raw descriptor of every kept
// feature and pooling scale.  The project's own source; it includes covdet.h and sift.h alone and is compiled against the
// reference's VLFeat sources by tools/make_covdet_golden.py, into a temporary directory.
//
//   usage: covdet_golden_driver request.bin result.bin [affine]
//   With the third argument (the word affine) the one call at sift.cc:467-473 is vl_covdet_extract_affine_shape instead of
//   vl_covdet_extract_orientations -- estimate_affine_shape = true -- and the third list holds the adapted features; everything
//   else is the same.  Without it the output is what it always was.
//   request: int32 width, height, octave_resolution, first_octave, max_num_features, upright, domain_size_pooling,
//            dsp_num_scales; double peak_threshold, edge_threshold, dsp_min_scale, dsp_max_scale; width * height grey bytes
//   result:  int32 n_detected, n_suppressed (VLFeat's counter), n_after_suppression, n_oriented, n_kept, num_scales, 0, 0;
//            double seconds (detection, orientations and descriptors; no file I/O); then four feature lists (detected, after
//            suppression, oriented, sorted) of 12 words a feature: float x, y, a11, a12, a21, a22; int32 o, s; float
//            peakScore, edgeScore, orientationScore; int32 index before the sort.  Then float raw[n_kept][num_scales][128].
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <limits>
#include <vector>

extern "C" {
#include "covdet.h"
#include "imopv.h"
#include "sift.h"
}

namespace {

void write_features(FILE* out, const VlCovDetFeature* f, int n) {
  for (int i = 0; i < n; ++i) {
    float w[6] = {f[i].frame.x, f[i].frame.y, f[i].frame.a11, f[i].frame.a12, f[i].frame.a21, f[i].frame.a22};
    int32_t os[2] = {(int32_t)f[i].o, (int32_t)f[i].s};
    float sc[3] = {f[i].peakScore, f[i].edgeScore, f[i].orientationScore};
    int32_t idx = (int32_t)f[i].laplacianScaleScore;  // the tag set below: unused by the DoG method
    fwrite(w, 4, 6, out);
    fwrite(os, 4, 2, out);
    fwrite(sc, 4, 3, out);
    fwrite(&idx, 4, 1, out);
  }
}

VlCovDet* detector(const int32_t* hdr, const double* thr, const std::vector<float>& data, bool suppress) {
  VlCovDet* covdet = vl_covdet_new(VL_COVDET_METHOD_DOG);
  vl_covdet_set_first_octave(covdet, hdr[3]);
  vl_covdet_set_octave_resolution(covdet, hdr[2]);
  vl_covdet_set_peak_threshold(covdet, thr[0]);
  vl_covdet_set_edge_threshold(covdet, thr[1]);
  if (!suppress) vl_covdet_set_non_extrema_suppression_threshold(covdet, 0.0);
  vl_covdet_put_image(covdet, data.data(), hdr[0], hdr[1]);
  vl_covdet_detect(covdet, hdr[4]);
  return covdet;
}

double now() {
  timespec t;
  clock_gettime(CLOCK_MONOTONIC, &t);
  return t.tv_sec + 1e-9 * t.tv_nsec;
}

}  // namespace

int main(int argc, char** argv) {
  int32_t hdr[8];
  double thr[4];
  if (argc != 3 && argc != 4) return 2;
  const bool affine = argc == 4;
  if (affine && strcmp(argv[3], "affine") != 0) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(hdr, 4, 8, f) != 8 || fread(thr, 8, 4, f) != 4) return 3;
  const size_t n = (size_t)hdr[0] * (size_t)hdr[1];
  std::vector<unsigned char> bytes(n);
  std::vector<float> data(n);
  if (fread(bytes.data(), 1, n, f) != n) return 3;
  fclose(f);
  for (size_t i = 0; i < n; ++i) data[i] = static_cast<float>(bytes[i]) / 255.0f;  // sift.cc:459
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 4;
  int32_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double seconds = 0.0;
  fwrite(counts, 4, 8, out);
  fwrite(&seconds, 8, 1, out);

  VlCovDet* raw = detector(hdr, thr, data, false);
  counts[0] = (int32_t)vl_covdet_get_num_features(raw);
  write_features(out, vl_covdet_get_features(raw), counts[0]);
  vl_covdet_delete(raw);

  const double t0 = now();
  VlCovDet* covdet = detector(hdr, thr, data, true);
  counts[1] = (int32_t)vl_covdet_get_num_non_extrema_suppressed(covdet);
  counts[2] = (int32_t)vl_covdet_get_num_features(covdet);
  write_features(out, vl_covdet_get_features(covdet), counts[2]);
  if (!hdr[5]) {  // sift.cc:467-473
    if (affine)
      vl_covdet_extract_affine_shape(covdet);
    else
      vl_covdet_extract_orientations(covdet);
  }
  const int num_features = (int)vl_covdet_get_num_features(covdet);
  VlCovDetFeature* features = (VlCovDetFeature*)vl_covdet_get_features(covdet);
  counts[3] = num_features;
  for (int i = 0; i < num_features; ++i) features[i].laplacianScaleScore = (float)i;
  write_features(out, features, num_features);
  const double t1 = now();

  std::sort(features, features + num_features, [](const VlCovDetFeature& feature1, const VlCovDetFeature& feature2) {  // sift.cc:479-487
    if (feature1.o == feature2.o) {
      return feature1.s > feature2.s;
    } else {
      return feature1.o > feature2.o;
    }
  });
  write_features(out, features, num_features);

  // the cut (sift.cc:489-513)
  const int kMaxOctaveResolution = 1000;
  const size_t max_num_features = (size_t)hdr[4];
  size_t kept = 0;
  int prev_octave_scale_idx = std::numeric_limits<int>::max();
  for (int i = 0; i < num_features; ++i) {
    ++kept;
    const int octave_scale_idx = (int)features[i].o * kMaxOctaveResolution + (int)features[i].s;
    if (octave_scale_idx != prev_octave_scale_idx && kept >= max_num_features) break;
    prev_octave_scale_idx = octave_scale_idx;
  }
  counts[4] = (int32_t)kept;

  // the descriptors (sift.cc:515-573)
  const size_t kPatchResolution = 15;
  const size_t kPatchSide = 2 * kPatchResolution + 1;
  const double kPatchRelativeExtent = 7.5;
  const double kPatchRelativeSmoothing = 1;
  const double kPatchStep = kPatchRelativeExtent / kPatchResolution;
  const double kSigma = kPatchRelativeExtent / (3.0 * (4 + 1) / 2) / kPatchStep;
  std::vector<float> patch(kPatchSide * kPatchSide);
  std::vector<float> patchXY(2 * kPatchSide * kPatchSide);
  float dsp_min_scale = 1;
  float dsp_scale_step = 0;
  int dsp_num_scales = 1;
  if (hdr[6]) {
    dsp_min_scale = thr[2];
    dsp_scale_step = (thr[3] - thr[2]) / hdr[7];
    dsp_num_scales = hdr[7];
  }
  counts[5] = dsp_num_scales;
  std::vector<float> scaled((size_t)dsp_num_scales * 128);
  VlSiftFilt* sift = vl_sift_new(16, 16, 1, 3, 0);
  vl_sift_set_magnif(sift, 3.0);
  const double t2 = now();
  for (size_t i = 0; i < kept; ++i) {
    for (int s = 0; s < dsp_num_scales; ++s) {
      const double dsp_scale = dsp_min_scale + s * dsp_scale_step;
      VlFrameOrientedEllipse scaled_frame = features[i].frame;
      scaled_frame.a11 *= dsp_scale;
      scaled_frame.a12 *= dsp_scale;
      scaled_frame.a21 *= dsp_scale;
      scaled_frame.a22 *= dsp_scale;
      vl_covdet_extract_patch_for_frame(covdet, patch.data(), kPatchResolution, kPatchRelativeExtent, kPatchRelativeSmoothing, scaled_frame);
      vl_imgradient_polar_f(patchXY.data(), patchXY.data() + 1, 2, 2 * kPatchSide, patch.data(), kPatchSide, kPatchSide, kPatchSide);
      // a row the bound check of vl_sift_calc_raw_descriptor left alone would show as zeros (it cannot trigger at the centre)
      memset(scaled.data() + (size_t)s * 128, 0, 512);
      vl_sift_calc_raw_descriptor(sift, patchXY.data(), scaled.data() + (size_t)s * 128, kPatchSide, kPatchSide, kPatchResolution,
                                  kPatchResolution, kSigma, 0);
    }
    const double t3 = now();  // the write is not part of the timed span
    fwrite(scaled.data(), 4, scaled.size(), out);
    seconds -= now() - t3;
  }
  seconds += (now() - t2) + (t1 - t0);
  fseek(out, 0, SEEK_SET);
  fwrite(counts, 4, 8, out);
  fwrite(&seconds, 8, 1, out);
  fclose(out);
  vl_sift_delete(sift);
  vl_covdet_delete(covdet);
  return 0;
}
