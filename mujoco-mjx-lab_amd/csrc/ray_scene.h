// What the renderer (render_kernels.hip) and the ray casts (ray_kernels.hip) share: the closed-form
// ray / plane, ray / sphere and ray / capsule tests on a geom's scene record.
// Quadratics are solved from the perpendicular offset at the ray's closest approach (|q|^2 against
// r^2), not as b^2 - 4ac on raw coordinates: with the camera 3 m from a 5 cm capsule the raw form
// loses four digits to cancellation.
// Included after step_kernels.hip (INL, f32x4).
#pragma once

namespace mjl {

// Ray (origin o, unit direction d) against a sphere, oc = o - centre: parameter of the first crossing at
// or past tmin (the far one when the near one lies before tmin), +inf for a miss.
INL float ray_sphere(const float* oc, const float* d, float r, float tmin) {
  const float b = -(oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2]);  // closest approach
  const float q0 = oc[0] + b * d[0], q1 = oc[1] + b * d[1], q2 = oc[2] + b * d[2];
  const float disc = r * r - (q0 * q0 + q1 * q1 + q2 * q2);
  if (disc < 0.f) return INFINITY;
  const float th = sqrtf(disc), t0 = b - th;
  return t0 >= tmin ? t0 : b + th;
}

// Ray against one geom record (A = centre, radius; B = z axis, half length): the hit parameter in
// [tmin, tmax], or +inf.
INL float ray_geom(const f32x4 A, const f32x4 B, const float* o, const float* d, float tmin, float tmax) {
  const float a[3] = {B.x, B.y, B.z};
  const float oc[3] = {o[0] - A.x, o[1] - A.y, o[2] - A.z};
  float t = INFINITY;
  if (A.w < 0.f) {  // plane through the centre, normal = z axis
    const float den = a[0] * d[0] + a[1] * d[1] + a[2] * d[2];
    if (fabsf(den) > 1e-9f) t = -(a[0] * oc[0] + a[1] * oc[1] + a[2] * oc[2]) / den;
  } else if (B.w == 0.f) {
    t = ray_sphere(oc, d, A.w, tmin);
  } else {  // capsule: cylinder side between the cap centres, and the outer half of each cap sphere
    const float r = A.w, h = B.w;
    const float da = d[0] * a[0] + d[1] * a[1] + d[2] * a[2], oa = oc[0] * a[0] + oc[1] * a[1] + oc[2] * a[2];
    const float dp[3] = {d[0] - da * a[0], d[1] - da * a[1], d[2] - da * a[2]};
    const float op[3] = {oc[0] - oa * a[0], oc[1] - oa * a[1], oc[2] - oa * a[2]};
    const float A2 = dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2];
    if (A2 > 1e-12f) {
      const float tm = -(op[0] * dp[0] + op[1] * dp[1] + op[2] * dp[2]) / A2;
      const float q0 = op[0] + tm * dp[0], q1 = op[1] + tm * dp[1], q2 = op[2] + tm * dp[2];
      const float disc = r * r - (q0 * q0 + q1 * q1 + q2 * q2);
      if (disc >= 0.f) {
        const float th = sqrtf(disc / A2), t0 = tm - th;
        const float ts = t0 >= tmin ? t0 : tm + th;
        if (fabsf(oa + ts * da) <= h && ts >= tmin && ts <= tmax) t = ts;
      }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const float sg = k ? -1.f : 1.f;
      const float occ[3] = {oc[0] - sg * h * a[0], oc[1] - sg * h * a[1], oc[2] - sg * h * a[2]};
      const float tc = ray_sphere(occ, d, r, tmin);
      if (sg * (oa + tc * da) >= h && tc >= tmin && tc <= tmax && tc < t) t = tc;
    }
  }
  return (t >= tmin && t <= tmax) ? t : INFINITY;
}

}  // namespace mjl
