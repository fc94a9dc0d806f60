// The smooth-L1 element shared by the RetinaNet / CenterNet loss kernels (det_targets.hip,
// retina_atss.hip).  Internal header: not part of the C ABI.
#pragma once
#include "cvl_common.h"

// one (discontinuous, Q8) smooth-L1 element, delta 1: returns the loss, *g = d loss / d pred
__device__ __forceinline__ float sl1_elem(float t, float x, float* g) {
  const float d = t - x;
  const float ad = fabsf(d);
  if (ad < 1.0f) { *g = -d; return 0.5f * d * d; }
  *g = d > 0.f ? -1.0f : (d < 0.f ? 1.0f : 0.0f);
  return ad;
}
