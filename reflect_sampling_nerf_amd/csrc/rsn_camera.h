// The camera ray of a pixel (include/rsn.h, "standalone data path" and "captures"): one device function for every kernel that needs
// it, so that equal (pose, camera, y, x) give bit-identical rays in rsn_sample_camera_rays, rsn_camera_rays_image, the pyramid and
// capture samplers and the point-cloud calls.
#pragma once
#include "rsn_common.h"

struct Intrinsics {
  float fx, fy, cx, cy;
};

// One row of a capture's camera table (include/rsn.h, "captures"): the pinhole part and the OpenCV / COLMAP coefficients.
struct Camera {
  Intrinsics k;
  float k1, k2, k3, p1, p2;
};

__device__ __forceinline__ Camera load_camera(const float* __restrict__ row) {
  return Camera{Intrinsics{row[0], row[1], row[2], row[3]}, row[4], row[5], row[6], row[7], row[8]};
}

// The ray whose camera-space direction is v = (vx, vy, -1), rotated by c2w[:, :3] and normalised; origin = c2w[:, 3].  pixel_area =
// |d - d_x1| |d - d_y1| with d_x1 / d_y1 the normalised directions of the x+1 / y+1 neighbours, whose camera-space directions are
// v + (exx, exy, 0) and v + (eyx, eyy, 0).  Those differences are formed without cancellation: with w = R v, g = R e (e = the
// neighbour's camera-space offset), a = |w|, b = |w + g|:  w/a - (w+g)/b = w (b - a)/(a b) - g/b,  b - a = (2 w.g + g.g) / (a + b).
// AXIS: the offsets are (exx, 0) and (0, eyy) (a pinhole camera); exy and eyx are not read, and the arithmetic is the pinhole
// function's as it always was.
// The tail every ray shares: w = R v and the neighbours' rotated offsets gx, gy -> direction, origin and pixel_area by the
// rearrangement above.
__device__ __forceinline__ void ray_from_rotated(const float* R, const float* w, const float* gx, const float* gy, float* o, float* d,
                                                 float* area) {
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

template <bool AXIS>
__device__ __forceinline__ void camera_ray_at(const float* __restrict__ c2w, float vx, float vy, float exx, float exy, float eyx,
                                              float eyy, float* o, float* d, float* area) {
  float R[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) R[j] = c2w[j];
  float w[3], gx[3], gy[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    w[i] = vx * R[4 * i + 0] + vy * R[4 * i + 1] + (-1.0f) * R[4 * i + 2];
    if (AXIS) {
      gx[i] = exx * R[4 * i + 0];
      gy[i] = eyy * R[4 * i + 1];
    } else {
      gx[i] = exx * R[4 * i + 0] + exy * R[4 * i + 1];
      gy[i] = eyx * R[4 * i + 0] + eyy * R[4 * i + 1];
    }
  }
  ray_from_rotated(R, w, gx, gy, o, d, area);
}

// camera_ray_at for a camera-space direction v and neighbour offsets ex, ey with three components each: a fisheye pixel beyond
// 90 degrees from the axis has v.z > 0, and its neighbours differ from it in z too.
__device__ __forceinline__ void camera_ray_at3(const float* __restrict__ c2w, const float* v, const float* ex, const float* ey, float* o,
                                               float* d, float* area) {
  float R[12];
#pragma unroll
  for (int j = 0; j < 12; ++j) R[j] = c2w[j];
  float w[3], gx[3], gy[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    w[i] = v[0] * R[4 * i + 0] + v[1] * R[4 * i + 1] + v[2] * R[4 * i + 2];
    gx[i] = ex[0] * R[4 * i + 0] + ex[1] * R[4 * i + 1] + ex[2] * R[4 * i + 2];
    gy[i] = ey[0] * R[4 * i + 0] + ey[1] * R[4 * i + 1] + ey[2] * R[4 * i + 2];
  }
  ray_from_rotated(R, w, gx, gy, o, d, area);
}

// nerfstudio 0.3 Cameras._generate_rays_from_coords, perspective: the pixel centre's camera-space direction
// v = ((x+.5-cx)/fx, -(y+.5-cy)/fy, -1); the neighbours' camera-space offsets are (1/fx, 0, 0) and (0, -1/fy, 0).
__device__ __forceinline__ void camera_ray(const float* __restrict__ c2w, Intrinsics k, int y, int x, float* o, float* d,
                                           float* area) {
  const float vx = ((float)x + 0.5f - k.cx) / k.fx;
  const float vy = -(((float)y + 0.5f - k.cy) / k.fy);
  const float ex = 1.0f / k.fx, ey = -(1.0f / k.fy);
  camera_ray_at<true>(c2w, vx, vy, ex, 0.0f, 0.0f, ey, o, d, area);
}

// The undistorted normalised point (X, Y) whose image under the OpenCV model (include/rsn.h, "captures") is (xd, yd): Newton on the
// 2 x 2 system from (xd, yd), exactly 10 iterations, none of them skipped early; an iteration whose |det J| <= 1e-12 leaves the
// point where it is.  fp64: the neighbours' offsets below are differences of two such points.  Nothing here checks convergence (the
// loader does, on the host, before a run starts).
__device__ __forceinline__ void undistort_point(const Camera& c, double xd, double yd, double* X, double* Y) {
  const double k1 = c.k1, k2 = c.k2, k3 = c.k3, p1 = c.p1, p2 = c.p2;
  double x = xd, y = yd;
#pragma unroll 1
  for (int it = 0; it < 10; ++it) {
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    const double drad = k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3));  // d rad / d r2
    const double rx = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x) - xd;
    const double ry = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y - yd;
    const double j11 = rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x;
    const double j12 = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y;  // = j21
    const double j22 = rad + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x;
    const double det = j11 * j22 - j12 * j12;
    if (fabs(det) > 1e-12) {
      x -= (j22 * rx - j12 * ry) / det;
      y -= (j11 * ry - j12 * rx) / det;
    }
  }
  *X = x;
  *Y = y;
}

// The ray of pixel (y, x) of a camera-table row.  All five coefficients exactly zero: camera_ray, unchanged.  Otherwise the pixel
// centre and its x+1 / y+1 neighbours are undistorted by their own solves; the centre's camera-space direction is (X, -Y, -1) and
// the neighbours' offsets are differences of the solved points, formed in fp64 and rounded to fp32 once.
__device__ __forceinline__ void capture_ray(const float* __restrict__ c2w, const Camera& c, int y, int x, float* o, float* d,
                                            float* area) {
  if (c.k1 == 0.0f && c.k2 == 0.0f && c.k3 == 0.0f && c.p1 == 0.0f && c.p2 == 0.0f) {
    camera_ray(c2w, c.k, y, x, o, d, area);
    return;
  }
  const double fx = c.k.fx, fy = c.k.fy, cx = c.k.cx, cy = c.k.cy;
  const double xd0 = ((double)x + 0.5 - cx) / fx, yd0 = ((double)y + 0.5 - cy) / fy;
  const double xd1 = ((double)x + 1.5 - cx) / fx, yd1 = ((double)y + 1.5 - cy) / fy;
  double X0, Y0, Xx, Yx, Xy, Yy;
  undistort_point(c, xd0, yd0, &X0, &Y0);
  undistort_point(c, xd1, yd0, &Xx, &Yx);
  undistort_point(c, xd0, yd1, &Xy, &Yy);
  camera_ray_at<false>(c2w, (float)X0, (float)(-Y0), (float)(Xx - X0), (float)(-(Yx - Y0)), (float)(Xy - X0), (float)(-(Yy - Y0)),
                       o, d, area);
}

// One row of a 9- or 12-column camera table (include/rsn.h, "captures: masks and fisheye lenses"): 12 columns add k4 and the model
// (0: the perspective arithmetic above, else OpenCV's equidistant fisheye); a 9-column row is a perspective one.
struct LensCamera {
  Camera c;
  float k4;
  bool fisheye;
};

__device__ __forceinline__ LensCamera load_lens_camera(const float* __restrict__ row, int stride) {
  LensCamera lc{load_camera(row), 0.0f, false};
  if (stride == 12) {
    lc.k4 = row[9];
    lc.fisheye = row[10] != 0.0f;
  }
  return lc;
}

// The camera-space unit direction of the distorted normalised point (xd, yd) of a fisheye row, all of it in fp64: theta solves
// theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = theta_d = |(xd, yd)| by Newton from theta_d, exactly 10 steps, none
// skipped early, a step whose |derivative| <= 1e-12 leaves theta where it is; theta is clipped to [0, pi].
__device__ __forceinline__ void fisheye_direction(const LensCamera& lc, double xd, double yd, double* v) {
  const double k1 = lc.c.k1, k2 = lc.c.k2, k3 = lc.c.k3, k4 = lc.k4;
  const double td = sqrt(xd * xd + yd * yd);
  double th = td;
#pragma unroll 1
  for (int it = 0; it < 10; ++it) {
    const double t2 = th * th;
    const double f = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - td;
    const double df = 1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))));
    if (fabs(df) > 1e-12) th -= f / df;
  }
  th = fmin(fmax(th, 0.0), 3.141592653589793);
  if (td == 0.0) {
    v[0] = 0.0, v[1] = 0.0, v[2] = -1.0;
    return;
  }
  const double s = sin(th) / td;
  v[0] = xd * s, v[1] = -(yd * s), v[2] = -cos(th);
}

// The ray of pixel (y, x) of a fisheye row: the centre and its x+1 / y+1 neighbours get their own solves; the neighbours' offsets
// are differences of the solved directions, formed in fp64 and rounded to fp32 once.
__device__ __forceinline__ void fisheye_ray(const float* __restrict__ c2w, const LensCamera& lc, int y, int x, float* o, float* d,
                                            float* area) {
  const double fx = lc.c.k.fx, fy = lc.c.k.fy, cx = lc.c.k.cx, cy = lc.c.k.cy;
  const double xd0 = ((double)x + 0.5 - cx) / fx, yd0 = ((double)y + 0.5 - cy) / fy;
  const double xd1 = ((double)x + 1.5 - cx) / fx, yd1 = ((double)y + 1.5 - cy) / fy;
  double v0[3], vx[3], vy[3];
  fisheye_direction(lc, xd0, yd0, v0);
  fisheye_direction(lc, xd1, yd0, vx);
  fisheye_direction(lc, xd0, yd1, vy);
  float v[3], ex[3], ey[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    v[j] = (float)v0[j];
    ex[j] = (float)(vx[j] - v0[j]);
    ey[j] = (float)(vy[j] - v0[j]);
  }
  camera_ray_at3(c2w, v, ex, ey, o, d, area);
}

// The ray of pixel (y, x) of a row of either table: a perspective row runs capture_ray unchanged.
__device__ __forceinline__ void lens_ray(const float* __restrict__ c2w, const LensCamera& lc, int y, int x, float* o, float* d,
                                         float* area) {
  if (lc.fisheye)
    fisheye_ray(c2w, lc, y, x, o, d, area);
  else
    capture_ray(c2w, lc.c, y, x, o, d, area);
}
