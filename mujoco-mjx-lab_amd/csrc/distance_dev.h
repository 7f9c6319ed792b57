// Device code of the geom distance readout that more than one kernel runs: the closed forms of a pair of scene
// records (dist_pair) and one entry of the gradient row of a staged pair (dist_jac_entry). geom_distance_kernel
// (distance_kernels.hip) and the whole-body instantiation of ik_kernel (ik_kernels.hip) call these, so a pair's
// dist and jac are the same bits in both.
// Included after step_kernels.hip (small math, f32x4) and dyn_kernels.hip (DynTab).
#pragma once

namespace mjl {

constexpr int kDistStage = 12;  // floats per staged pair: from, to, normal, body1, body2, live

// the point of the axis segment (centre c, unit axis z, half length h) nearest to p
static INL void dist_seg_point(float* r, const float* c, const float* z, float h, const float* p) {
  const float d[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const float t = fminf(fmaxf(dot3(d, z), -h), h);
  for (int i = 0; i < 3; i++) r[i] = c[i] + t * z[i];
}

// Signed distance of geom records (A1, B1) and (A2, B2), not both planes: `from` on geom 1's surface, `to` on
// geom 2's, n the unit vector from geom 1 towards geom 2, to = from + dist n.
static INL float dist_pair(const f32x4 A1, const f32x4 B1, const f32x4 A2, const f32x4 B2, float* from, float* to,
                           float* n) {
  const bool swap = A2.w < 0.f;  // the plane first
  const f32x4 Pa = swap ? A2 : A1, Pb = swap ? B2 : B1, Qa = swap ? A1 : A2, Qb = swap ? B1 : B2;
  const float x1[3] = {Pa.x, Pa.y, Pa.z}, z1[3] = {Pb.x, Pb.y, Pb.z};
  const float x2[3] = {Qa.x, Qa.y, Qa.z}, z2[3] = {Qb.x, Qb.y, Qb.z};
  const float r2 = Qa.w, h2 = Qb.w;
  float dist, pa[3], pb[3];
  if (Pa.w < 0.f) {  // half-space z1 . (x - x1) <= 0 against a sphere or capsule
    const float c[3] = {x2[0] - x1[0], x2[1] - x1[1], x2[2] - x1[2]};
    const float dc = dot3(c, z1), dz = h2 * dot3(z2, z1);
    const float sg = dz > 0.f ? -1.f : 1.f;  // the end nearer to the plane (a tie: +z)
    dist = (dc + sg * dz) - r2;
    for (int i = 0; i < 3; i++) {
      n[i] = z1[i];
      pb[i] = x2[i] + sg * h2 * z2[i] - r2 * z1[i];
      pa[i] = pb[i] - dist * z1[i];
    }
  } else {
    const float r1 = Pa.w, h1 = Pb.w;
    const float w[3] = {x1[0] - x2[0], x1[1] - x2[1], x1[2] - x2[2]};
    float cr[3], wc[3];
    cross3(cr, z1, z2);
    cross3(wc, w, z2);
    const float den = dot3(cr, cr);
    const float s = den < 1e-12f ? 0.f : -dot3(wc, cr) / den;  // the lines' closest approach, on line 1
    const float t = fminf(fmaxf(s, -h1), h1);
    float q1[3], c1[3], c2[3];
    for (int i = 0; i < 3; i++) q1[i] = x1[i] + t * z1[i];
    dist_seg_point(c2, x2, z2, h2, q1);
    dist_seg_point(c1, x1, z1, h1, c2);
    float v[3] = {c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]};
    const float d2 = dot3(v, v);
    float d = 0.f;
    if (d2 > 1e-30f) {
      d = sqrtf(d2);
      const float inv = 1.f / d;
      for (int i = 0; i < 3; i++) v[i] *= inv;
    } else {  // coincident axis points: no direction is defined, world +z is taken
      v[0] = 0.f; v[1] = 0.f; v[2] = 1.f;
    }
    dist = d - (r1 + r2);
    for (int i = 0; i < 3; i++) {
      n[i] = v[i];
      pa[i] = c1[i] + r1 * v[i];
      pb[i] = c2[i] - r2 * v[i];
    }
  }
  for (int i = 0; i < 3; i++) {
    from[i] = swap ? pb[i] : pa[i];
    to[i] = swap ? pa[i] : pb[i];
    n[i] = swap ? -n[i] : n[i];
  }
  return dist;
}

// Entry d of the gradient row of the live pair staged at s (kDistStage floats): normal . (column d of
// jacp(to, body2) - column d of jacp(from, body1)), the dof's axis and anchor (dyn_dof_axis) in ax / an.
static INL float dist_jac_entry(const DynTab* tab, const float* s, int d, int kind, const float* ax,
                                const float* an) {
  const int b1 = __float_as_int(s[9]), b2 = __float_as_int(s[10]);
  const float n[3] = {s[6], s[7], s[8]};
  float cf[3] = {0.f, 0.f, 0.f}, ct[3] = {0.f, 0.f, 0.f};
  if ((tab->body_dofmask[b1] >> d) & 1u) {
    if (kind == 1) {
      for (int i = 0; i < 3; i++) cf[i] = ax[i];
    } else {
      const float r[3] = {s[0] - an[0], s[1] - an[1], s[2] - an[2]};
      cross3(cf, ax, r);
    }
  }
  if ((tab->body_dofmask[b2] >> d) & 1u) {
    if (kind == 1) {
      for (int i = 0; i < 3; i++) ct[i] = ax[i];
    } else {
      const float r[3] = {s[3] - an[0], s[4] - an[1], s[5] - an[2]};
      cross3(ct, ax, r);
    }
  }
  const float df[3] = {ct[0] - cf[0], ct[1] - cf[1], ct[2] - cf[2]};
  return dot3(n, df);
}

}  // namespace mjl
