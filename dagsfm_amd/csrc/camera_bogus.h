// camera_bogus.h -- CameraModelHasBogusParams (src/base/camera_models.h:473-528) on the host, shared by the stages that
// judge cameras (re-triangulation, the point filters).
#ifndef DAGSFM_AMD_CSRC_CAMERA_BOGUS_H_
#define DAGSFM_AMD_CSRC_CAMERA_BOGUS_H_

#include <algorithm>
#include <cmath>

#include "../../include/dagsfm_mi355x.h"
#include "verify_camera.h"

// the verdict, with the smallest margin of its tests folded into *margin: the ratio tests relative to their bounds
inline bool cam_has_bogus_params(const dsm_camera& c, double min_ratio, double max_ratio, double max_extra, double* margin) {
  const int id = c.model_id;
  const bool two = cam_two_focal(id);
  const int pp = two ? 2 : 1, nf = two ? 2 : 1;
  const double cx = c.params[pp], cy = c.params[pp + 1];
  if (cx < 0 || cx > (double)c.width || cy < 0 || cy > (double)c.height) return true;
  const double max_size = (double)std::max(c.width, c.height);
  for (int i = 0; i < nf; ++i) {
    const double ratio = c.params[i] / max_size;
    *margin = std::min({*margin, std::fabs(ratio - min_ratio) / min_ratio, std::fabs(ratio - max_ratio) / max_ratio});
    if (ratio < min_ratio || ratio > max_ratio) return true;
  }
  const int first_extra = (id == 0 || id == 1) ? cam_num_params(id) : (two ? 4 : 3);
  for (int i = first_extra; i < cam_num_params(id); ++i) {
    if (max_extra > 0) *margin = std::min(*margin, std::fabs(std::fabs(c.params[i]) - max_extra) / max_extra);
    if (std::fabs(c.params[i]) > max_extra) return true;
  }
  return false;
}

#endif  // DAGSFM_AMD_CSRC_CAMERA_BOGUS_H_
