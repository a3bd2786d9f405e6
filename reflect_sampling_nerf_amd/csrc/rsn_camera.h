// The camera ray of a pixel (include/rsn.h, "standalone data path"): one device function for every kernel that needs it, so that
// equal (pose, intrinsics, y, x) give bit-identical rays in rsn_sample_camera_rays, rsn_camera_rays_image and the point-cloud calls.
#pragma once
#include "rsn_common.h"

struct Intrinsics {
  float fx, fy, cx, cy;
};

// nerfstudio 0.3 Cameras._generate_rays_from_coords, perspective: the pixel centre's camera-space direction
// v = ((x+.5-cx)/fx, -(y+.5-cy)/fy, -1), rotated by c2w[:, :3] and normalised; origin = c2w[:, 3].  pixel_area =
// |d - d_x1| |d - d_y1| with d_x1 / d_y1 the normalised directions of the x+1 / y+1 neighbours.  Those differences are
// formed without cancellation: with w = R v, g = R e (e = the neighbour's camera-space offset, (1/fx, 0, 0) or
// (0, -1/fy, 0)), a = |w|, b = |w + g|:  w/a - (w+g)/b = w (b - a)/(a b) - g/b,  b - a = (2 w.g + g.g) / (a + b).
__device__ __forceinline__ void camera_ray(const float* __restrict__ c2w, Intrinsics k, int y, int x, float* o, float* d,
                                           float* area) {
  float R[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) R[j] = c2w[j];
  const float vx = ((float)x + 0.5f - k.cx) / k.fx;
  const float vy = -(((float)y + 0.5f - k.cy) / k.fy);
  float w[3], gx[3], gy[3];
  const float ex = 1.0f / k.fx, ey = -(1.0f / k.fy);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    w[i] = vx * R[4 * i + 0] + vy * R[4 * i + 1] + (-1.0f) * R[4 * i + 2];
    gx[i] = ex * R[4 * i + 0];
    gy[i] = ey * R[4 * i + 1];
  }
  const float a2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  const float a = sqrtf(a2);
  float nb[2];
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const float* g = n == 0 ? gx : gy;
    const float wg = w[0] * g[0] + w[1] * g[1] + w[2] * g[2];
    const float gg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    const float db2 = 2.0f * wg + gg;  // b^2 - a^2
    const float b = sqrtf(a2 + db2);
    const float bma = db2 / (a + b);
    const float s = bma / (a * b), t = 1.0f / b;
    const float e0 = w[0] * s - g[0] * t, e1 = w[1] * s - g[1] * t, e2 = w[2] * s - g[2] * t;
    nb[n] = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    d[i] = w[i] / a;
    o[i] = R[4 * i + 3];
  }
  *area = nb[0] * nb[1];
}
