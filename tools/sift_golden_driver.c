/* sift_golden_driver.c -- runs VLFeat's vl_sift over one grey image in the call sequence of COLMAP's ExtractSiftFeaturesCPU
 * (src/feature/sift.cc:266-385) and writes what VLFeat returned, untouched: every refined keypoint of every octave, its
 * orientations (double) and the 128 floats of the descriptor of each orientation.  The project's own source; it includes
 * sift.h alone and is compiled against the reference's VLFeat sources by tools/make_sift_golden.py, into a temporary directory.
 *
 *   usage: sift_golden_driver request.bin result.bin
 *   request: int32 width, height, num_octaves, octave_resolution, first_octave, upright, 0, 0; double peak_threshold,
 *            edge_threshold; width * height grey bytes
 *   result:  int32 count, 0; per keypoint int32 o, ix, iy, is; float x, y, s, sigma; int32 num_angles, 0; double angles[4];
 *            float descriptor[num_angles][128]
 * A descriptor row is zeroed before the call: where vl_sift_calc_keypoint_descriptor's bound check (sift.c:1976-1983) returns
 * early it leaves the row as it was. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sift.h"

int main(int argc, char** argv) {
  int32_t hdr[8];
  double thr[2];
  FILE* f;
  FILE* out;
  unsigned char* bytes;
  float* data;
  VlSiftFilt* sift;
  int first = 1, i, a;
  int32_t total = 0, zero = 0;
  size_t n;
  if (argc != 3) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(hdr, 4, 8, f) != 8 || fread(thr, 8, 2, f) != 2) return 3;
  n = (size_t)hdr[0] * (size_t)hdr[1];
  bytes = (unsigned char*)malloc(n);
  data = (float*)malloc(n * sizeof(float));
  if (fread(bytes, 1, n, f) != n) return 3;
  fclose(f);
  for (i = 0; i < (int)n; ++i) data[i] = (float)bytes[i] / 255.0f; /* sift.cc:288 */
  sift = vl_sift_new(hdr[0], hdr[1], hdr[2], hdr[3], hdr[4]);
  vl_sift_set_peak_thresh(sift, thr[0]);
  vl_sift_set_edge_thresh(sift, thr[1]);
  out = fopen(argv[2], "wb");
  if (!out) return 4;
  fwrite(&total, 4, 1, out);
  fwrite(&zero, 4, 1, out);
  for (;;) {
    VlSiftKeypoint const* keys;
    int nkeys;
    if (first) {
      if (vl_sift_process_first_octave(sift, data)) break;
      first = 0;
    } else if (vl_sift_process_next_octave(sift)) {
      break;
    }
    vl_sift_detect(sift);
    keys = vl_sift_get_keypoints(sift);
    nkeys = vl_sift_get_nkeypoints(sift);
    for (i = 0; i < nkeys; ++i) {
      double angles[4] = {0.0, 0.0, 0.0, 0.0};
      int32_t ints[4], na[2];
      float flts[4], desc[128];
      int num = 1;
      if (!hdr[5]) num = vl_sift_calc_keypoint_orientations(sift, angles, &keys[i]);
      ints[0] = keys[i].o;
      ints[1] = keys[i].ix;
      ints[2] = keys[i].iy;
      ints[3] = keys[i].is;
      flts[0] = keys[i].x;
      flts[1] = keys[i].y;
      flts[2] = keys[i].s;
      flts[3] = keys[i].sigma;
      na[0] = num;
      na[1] = 0;
      fwrite(ints, 4, 4, out);
      fwrite(flts, 4, 4, out);
      fwrite(na, 4, 2, out);
      fwrite(angles, 8, 4, out);
      for (a = 0; a < num; ++a) {
        memset(desc, 0, sizeof(desc));
        vl_sift_calc_keypoint_descriptor(sift, desc, &keys[i], angles[a]);
        fwrite(desc, 4, 128, out);
      }
      ++total;
    }
  }
  fseek(out, 0, SEEK_SET);
  fwrite(&total, 4, 1, out);
  fclose(out);
  vl_sift_delete(sift);
  free(data);
  free(bytes);
  return 0;
}
