// What the labelled epilogues share (labelstat.hip, labelhist.hip, labelpair.hip): the label of a voxel as it is read,
// and the rule that turns the largest magnitude of a volume into the power-of-two scales of its 64-bit fixed-point sums.
// Internal linkage, as valstat_device.h: each translation unit gets its own copy of what it uses.
#pragma once
#include <math.h>
#include <stdint.h>

namespace {

constexpr int kLabelMax = 4096;

// the label at element `at` of a label volume of 1 (uint8), 2 (int16) or 4 (int32) bytes per element; lab_bytes is
// uniform over a launch
__device__ __forceinline__ int label_read(const void* lab, int lab_bytes, int64_t at) {
  switch (lab_bytes) {
    case 1: return static_cast<const uint8_t*>(lab)[at];
    case 2: return static_cast<const int16_t*>(lab)[at];
    default: return static_cast<const int32_t*>(lab)[at];
  }
}

// nb = ceil(log2 numel)
__host__ __device__ inline int labelstat_bits(int64_t numel) {
  int nb = 0;
  while (nb < 62 && ((int64_t)1 << nb) < numel) ++nb;
  return nb;
}
inline __host__ __device__ int labelstat_clamp(int s) { return s < -1000 ? -1000 : (s > 1000 ? 1000 : s); }
// maxabs < 2^e (frexp), s = 61 - nb - e, so that numel * |v| 2^s <= 2^61; s2 likewise from the fp64 product
// maxabs * maxabs, which bounds every fl(v * v) (2 e where the product leaves the fp64 range)
__host__ __device__ inline void labelstat_scale_rule(double maxabs, int64_t numel, int* s, int* s2) {
  *s = *s2 = 0;
  if (!(maxabs > 0.0)) return;
  const int nb = labelstat_bits(numel);
  int e = 0, e2 = 0;
  frexp(maxabs, &e);
  const double sq = maxabs * maxabs;
  if (sq > 0.0 && sq <= 1.7976931348623157e308) frexp(sq, &e2); else e2 = 2 * e;
  *s = labelstat_clamp(61 - nb - e);
  *s2 = labelstat_clamp(61 - nb - e2);
}

}  // namespace
