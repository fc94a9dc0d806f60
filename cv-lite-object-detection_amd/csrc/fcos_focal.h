// The focal-loss terms shared by the FCOS loss kernels (fcos_loss.hip, fcos_paper.hip; the Quality Focal
// Loss term: fcos_gfl.hip, fcos_tal.hip).
// Internal header: not part of the C ABI.
#pragma once
#include "cvl_common.h"

// q^gamma: the reference default gamma = 2 as a product (the values every training path uses)
__device__ __forceinline__ float powg(float q, float gamma) { return gamma == 2.0f ? q * q : powf(q, gamma); }

// focal loss term (the reference's stable form, fcos.py:443-462) and d/dx:
//   y a q^g (L - min(x,0)) + (1-y)(1-a) p^g (L + max(x,0)),  p = sigmoid(x), q = 1 - p, L = log(1+e^-|x|)
//   d/dx = -y a q^g (g p nlp + q) + (1-y)(1-a) p^g (g q nlq + p)
__device__ __forceinline__ float focal_term(float y, float x, float alpha, float gamma, float* g) {
  const float e = expf(-fabsf(x));
  const float L = log1pf(e);                       // log(1 + exp(-|x|))
  const float p1 = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);   // sigmoid(x)
  const float q1 = x >= 0.f ? e / (1.0f + e) : 1.0f / (1.0f + e);   // 1 - sigmoid(x)
  const float nlp = L - fminf(x, 0.f);             // -log p
  const float nlq = L + fmaxf(x, 0.f);             // -log(1-p)
  const float qg = powg(q1, gamma), pg = powg(p1, gamma);
  const float wpos = y * alpha * qg;
  const float wneg = (1.0f - y) * (1.0f - alpha) * pg;
  *g = -wpos * (gamma * p1 * nlp + q1) + wneg * (gamma * q1 * nlq + p1);
  return wpos * nlp + wneg * nlq;
}

// Quality Focal Loss term |y - s|^beta BCE(x, y) and d/dx with y constant (beta = 2 as a product):
//   d/dx = beta |y - s|^(beta-1) sign(s - y) s (1 - s) BCE + |y - s|^beta (s - y)
__device__ __forceinline__ float qfl_term(float y, float x, float beta, float* g) {
  const float e = expf(-fabsf(x));
  const float s = x >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);     // sigmoid(x)
  const float q1 = x >= 0.f ? e / (1.0f + e) : 1.0f / (1.0f + e);    // 1 - sigmoid(x)
  const float bce = (fmaxf(x, 0.f) - x * y) + log1pf(e);
  const float df = s - y, a = fabsf(df);
  float mod, dmod;
  if (beta == 2.0f) {
    mod = a * a;
    dmod = 2.0f * df;
  } else {
    mod = powf(a, beta);
    dmod = a > 0.f ? beta * powf(a, beta - 1.0f) * (df > 0.f ? 1.0f : -1.0f) : 0.f;
  }
  *g = dmod * (s * q1) * bce + mod * df;
  return mod * bce;
}
