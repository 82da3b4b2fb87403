// ImageNormalize arithmetic shared by ud_image_normalize and the fused output of ud_image_affine, so the two paths
// cannot drift.  mmcv.imnormalize (third party): float32 image, optional channel reversal (cvtColor BGR2RGB),
// img - float32(mean), then * float32(1 / float64(std)), each rounded to float32 (no contraction).
#pragma once
#include <hip/hip_runtime.h>

struct UdNorm {
  float m0, m1, m2, s0, s1, s2;
  int to_rgb;
};

// mean / std: HOST float[3]; mmcv takes mean to float64 and stdinv = 1 / float64(std), OpenCV applies both in float32.
static inline UdNorm ud_norm_make(const float* mean, const float* std, int to_rgb) {
  UdNorm n;
  n.m0 = mean[0], n.m1 = mean[1], n.m2 = mean[2];
  n.s0 = (float)(1.0 / (double)std[0]), n.s1 = (float)(1.0 / (double)std[1]), n.s2 = (float)(1.0 / (double)std[2]);
  n.to_rgb = to_rgb ? 1 : 0;
  return n;
}

__device__ __forceinline__ void ud_norm_apply(const UdNorm& n, unsigned p0, unsigned p1, unsigned p2, float& v0,
                                              float& v1, float& v2) {
  v0 = (float)p0, v1 = (float)p1, v2 = (float)p2;
  if (n.to_rgb) {
    const float tmp = v0;
    v0 = v2;
    v2 = tmp;
  }
  v0 = __fmul_rn(__fsub_rn(v0, n.m0), n.s0);
  v1 = __fmul_rn(__fsub_rn(v1, n.m1), n.s1);
  v2 = __fmul_rn(__fsub_rn(v2, n.m2), n.s2);
}
