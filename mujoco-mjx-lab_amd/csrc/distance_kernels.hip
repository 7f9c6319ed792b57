// Geom distance readout (mjl_geom_distance): mj_geomDistance for npair caller-chosen geom pairs per env, signed,
// capped at distmax, with witness points, the normal and the gradient n' (jacp(to) - jacp(from)), as
// include/mjx355.h defines them.
//
// One launch, one 64-lane wavefront per (env, chunk of `chunk` pairs):
//   1. qpos into LDS; the positions-only tree pass of the Jacobian readout (dyn_tree_pass, dyn_kernels.hip): body
//      frames and the world axis / anchor of every hinge dof in LDS. The stored xpos / xquat are neither read nor
//      written. One pass serves both the geoms and the gradient, so dist / fromto / normal do not depend on
//      whether jac is asked for, bit for bit, and the gradient's columns are mjl_jac's.
//   2. lane = geom: the geom's scene record (scene_geom_record, ray_kernels.hip: centre, radius, z axis, half
//      length: 32 B) and its body id into LDS, at most MJL_MAXGEOM = 32 of them.
//   3. the chunk in tiles of 64 pairs, lane = pair: both ids are checked against ngeom before a record is read;
//      then one of two closed forms, chosen from the two records (a lane's branch depends on its pair only):
//        plane - sphere / capsule   the nearer end of the axis segment (a sphere's is its centre; a tie takes the
//                                   +z end), dist = (end - plane point) . normal - r
//        sphere / capsule pairs     the closest points of the two axis segments (a sphere's has half length 0):
//                                   the lines' closest approach on segment 1, clamped; its nearest point on
//                                   segment 2; that point's nearest on segment 1 (collide's clamp-and-reproject,
//                                   with exact projections; parallel axes, |z1 x z2|^2 < 1e-12, start from
//                                   segment 1's centre). dist = |pb - pa| - (r1 + r2)
//      dist, fromto and normal are stored by the pair's lane; with jac the tile's witness points, normals and
//      body ids are staged in LDS (3 KB).
//   4. jac: lane = dof in both halves of the wave (jac_kernel's layout), the dof's axis and anchor in registers;
//      the tile's pairs two at a time, the lower half taking pair p and the upper half p + 1, the staged pair
//      read at half-uniform LDS addresses. Lane d stores normal . (column d of jacp(to, body2) - column d of
//      jacp(from, body1)): consecutive lanes, consecutive floats of the pair's nv-wide row.
// chunk >= npair is "kinematics once per env"; a smaller chunk repeats steps 1 and 2 in every chunk's wavefront
// and gives the device more of them. The host picks the chunk (kDistChunk, capi.hip; DESIGN.md "Geom distance").
// An output passed as NULL costs neither staging nor stores (branches on the kernel arguments, uniform).
// The closed forms and the gradient entry are distance_dev.h's (the whole-body IK kernel runs them too).
// Included by capi.hip after dyn_kernels.hip and ray_kernels.hip.
#pragma once

#include "distance_dev.h"

namespace mjl {

struct DistArgs {
  const ModelF* m;      // the shared model block (no geometric field is per-env)
  const DynTab* tab;
  const float* qpos;    // [nenv, nq]
  const float* mask;    // [nenv] or null
  int nenv, npair, chunk, nchunk;
  const int32_t *geom1, *geom2;  // [npair]
  float distmax;
  float* dist;          // [nenv, npair]
  float* fromto;        // [nenv, npair, 6] or null
  float* normal;        // [nenv, npair, 3] or null
  float* jac;           // [nenv, npair, nv] or null
};

__global__ __launch_bounds__(64) void geom_distance_kernel(DistArgs A) {
  __shared__ float qpos[MJL_MAXQ];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float dax[MJL_MAXV][3], danc[MJL_MAXV][3];
  __shared__ f32x4 S4[2 * MJL_MAXGEOM];
  __shared__ int gbody[MJL_MAXGEOM];
  __shared__ float P[64 * kDistStage];  // the tile's pairs for the jac pass
  const MP m = uniform_ptr((MP)A.m);
  const int lane = threadIdx.x;
  const int env = blockIdx.x / A.nchunk, c = blockIdx.x % A.nchunk;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const int nq = min(m->nq, MJL_MAXQ), nv = min(m->nv, MJL_MAXV), nbody = min(m->nbody, MJL_MAXBODY);
  const int ngeom = min(m->ngeom, MJL_MAXGEOM), maxlevel = m->maxlevel, npair = A.npair;

  if (lane < nq) qpos[lane] = A.qpos[(size_t)env * nq + lane];
  if (lane == 0) {
    xquat[0][0] = 1.f; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.f;
    xpos[0][0] = xpos[0][1] = xpos[0][2] = 0.f;
  }
  if (lane < MJL_MAXV)
    for (int i = 0; i < 3; i++) dax[lane][i] = danc[lane][i] = 0.f;
  __syncthreads();
  const BodyRec br = ldrec(&m->brec[lane < nbody ? lane : 0]);
  dyn_tree_pass(m, br, qpos, xpos, xquat, dax, danc, nbody, maxlevel, lane);

  // ---- lane = geom: the scene record and the body
  if (lane < ngeom) {
    const FrameRec fr = ldrec(&m->frec[lane]);
    const int gb = max(0, min(fr.body, nbody - 1));
    float gm[9], rec[8];
    q2m(gm, xquat[gb]);
    scene_geom_record(m, lane, fr, gm, xpos[gb], rec);
    S4[2 * lane] = f32x4{rec[0], rec[1], rec[2], rec[3]};
    S4[2 * lane + 1] = f32x4{rec[4], rec[5], rec[6], rec[7]};
    gbody[lane] = gb;
  }
  __syncthreads();

  // ---- lane = dof in both halves of the wave (the jac pass)
  const int d = lane & 31, h = lane >> 5;
  const bool isd = d < nv;
  float ax[3] = {0.f, 0.f, 0.f}, an[3] = {0.f, 0.f, 0.f};
  int kind = 0;
  if (A.jac) {
    const DofRec dr = ldrec(&m->drec[isd ? d : 0]);
    kind = dyn_dof_axis(dr, isd ? d : 0, xpos, xquat, dax, danc, nbody, ax, an);
  }
  const float nan = __int_as_float(0x7fc00000);

  const int p1 = min(npair, (c + 1) * A.chunk);
  for (int t0 = c * A.chunk; t0 < p1; t0 += 64) {
    const int p = t0 + lane;
    if (p < p1) {
      const int g1 = A.geom1[p], g2 = A.geom2[p];
      bool ok = g1 >= 0 && g1 < ngeom && g2 >= 0 && g2 < ngeom && g1 != g2;
      const int s1 = ok ? g1 : 0, s2 = ok ? g2 : 0;
      const f32x4 A1 = S4[2 * s1], B1 = S4[2 * s1 + 1], A2 = S4[2 * s2], B2 = S4[2 * s2 + 1];
      ok = ok && !(A1.w < 0.f && A2.w < 0.f);
      float from[3] = {0.f, 0.f, 0.f}, to[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
      float dist = nan;
      bool live = false;
      if (ok) {
        dist = dist_pair(A1, B1, A2, B2, from, to, n);
        live = !(dist > A.distmax);
        if (!live) {
          dist = A.distmax;
          for (int i = 0; i < 3; i++) from[i] = to[i] = n[i] = 0.f;
        }
      }
      const size_t e = (size_t)env * npair + p;
      A.dist[e] = dist;
      if (A.fromto)
        for (int i = 0; i < 3; i++) { A.fromto[6 * e + i] = from[i]; A.fromto[6 * e + 3 + i] = to[i]; }
      if (A.normal)
        for (int i = 0; i < 3; i++) A.normal[3 * e + i] = n[i];
      if (A.jac) {
        float* s = P + lane * kDistStage;
        for (int i = 0; i < 3; i++) { s[i] = from[i]; s[3 + i] = to[i]; s[6 + i] = n[i]; }
        s[9] = __int_as_float(gbody[s1]);
        s[10] = __int_as_float(gbody[s2]);
        s[11] = live ? 1.f : 0.f;
      }
    }
    if (!A.jac) continue;
    __syncthreads();
    const int nt = min(64, p1 - t0);
    for (int k0 = 0; k0 < nt; k0 += 2) {
      const int k = k0 + h;
      if (k < nt && isd) {
        const float* s = P + k * kDistStage;
        float v = 0.f;
        if (s[11] != 0.f) v = dist_jac_entry(A.tab, s, d, kind, ax, an);
        A.jac[((size_t)env * npair + t0 + k) * nv + d] = v;
      }
    }
    __syncthreads();
  }
}

}  // namespace mjl
